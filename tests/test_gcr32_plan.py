"""csrc/gcr32_plan.h — the host plan of the low-precision GCR's fp32 matrix copy — against the numpy plan of tests/gcr32_cases.py, on the
CPU.  tests/cpp/gcr32_plan_check.cpp — a stand-alone program — is built with g++ and the address / undefined-behaviour sanitizers and
run on every case: width, real-slab detection, slab, tail and tile table bit for bit, the overflow refusal naming the row, the
inconsistent inputs and the parameter refusals."""
import os
import subprocess

import numpy as np
import pytest

from tests import gcr32_cases as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gcr32_plan") / "gcr32_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "gcr32_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return path


def run(exe, tmp_path, n, rowptr, col, val):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([n, col.size, g.TILE], np.int64).tofile(f)
        np.ascontiguousarray(rowptr, np.int64).tofile(f)
        np.ascontiguousarray(col, np.int64).tofile(f)
        np.ascontiguousarray(val, np.complex128).view(np.float64).tofile(f)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    return p.stdout.splitlines(), dst


def read_plan(path):
    with open(path, "rb") as f:
        W, npad, real, nt, tnnz, ntile, stored = (int(v) for v in np.fromfile(f, np.int64, 7))
        nc = 1 if real else 2
        d = dict(W=W, npad=npad, real=bool(real), stored=stored)
        d["ell_col"] = np.fromfile(f, np.int32, W * npad).reshape(W, npad)
        d["ell_val"] = np.fromfile(f, np.float32, W * npad * nc).reshape(W, npad, nc)
        d["tail_rows"] = np.fromfile(f, np.int32, nt)
        d["tail_ptr"] = np.fromfile(f, np.int32, nt + 1)
        d["tail_col"] = np.fromfile(f, np.int32, tnnz)
        d["tail_val"] = np.fromfile(f, np.float32, tnnz * nc).reshape(tnnz, nc)
        d["tile_tail"] = np.fromfile(f, np.int32, ntile)
        assert f.read() == b""
    return d


def parts(z, real):
    """a complex64 array as the float bits the plan stores"""
    z = np.ascontiguousarray(z, np.complex64)
    v = z.view(np.float32).reshape(z.shape + (2,))
    return v[..., :1] if real else v


@pytest.mark.parametrize("name", sorted(g.CASES))
def test_plan_equals_the_model(exe, tmp_path, name):
    c = g.case(name)
    p = g.plan(c)
    out, dst = run(exe, tmp_path, c.n, c.rowptr, c.col, c.val)
    assert out[0] == "OK %d %d %d" % (p.W, p.tail_rows.size, int(p.real)), out
    d = read_plan(dst)
    assert (d["W"], d["npad"], d["real"], d["stored"]) == (p.W, p.npad, p.real, p.stored_bytes)
    assert np.array_equal(d["ell_col"], p.ell_col)
    assert np.array_equal(d["ell_val"].view(np.uint32), parts(p.ell_val, p.real).view(np.uint32))
    for key in ("tail_rows", "tail_ptr", "tail_col", "tile_tail"):
        assert np.array_equal(d[key], getattr(p, key)), key
    assert np.array_equal(d["tail_val"].view(np.uint32), parts(p.tail_val, p.real).view(np.uint32))


def test_an_overflowing_value_is_refused_and_the_row_named(exe, tmp_path):
    c = g.case("g", None)
    assert g.bad_row(c) == g.G_ROW
    out, _ = run(exe, tmp_path, c.n, c.rowptr, c.col, c.val)
    assert out[0] == "INVALID" and ("row %d " % g.G_ROW) in out[1] and "single precision" in out[1], out


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 3.5e38, 1j * 1e39])
def test_values_outside_float_are_refused(exe, tmp_path, bad):
    c = g.case("f")
    val = c.val.copy()
    val[int(c.rowptr[20])] = bad
    out, _ = run(exe, tmp_path, c.n, c.rowptr, c.col, val)
    assert out[0] == "INVALID" and "row 20 " in out[1], out


def test_the_largest_float_is_taken(exe, tmp_path):
    c = g.case("f")
    val = c.val.copy()
    val[0] = float(np.finfo(np.float32).max)
    out, _ = run(exe, tmp_path, c.n, c.rowptr, c.col, val)
    assert out[0].startswith("OK"), out


def test_a_column_outside_the_square_and_a_decreasing_rowptr_are_refused(exe, tmp_path):
    c = g.case("f")
    col = c.col.copy()
    col[5] = c.n
    out, _ = run(exe, tmp_path, c.n, c.rowptr, col, c.val)
    assert out[0] == "INVALID" and "square" in out[1], out
    rp = c.rowptr.copy()
    rp[3] = rp[4] + 1
    out, _ = run(exe, tmp_path, c.n, rp, c.col, c.val)
    assert out[0] == "INVALID" and "rowptr" in out[1], out


def test_an_empty_matrix_and_empty_rows(exe, tmp_path):
    out, dst = run(exe, tmp_path, 0, np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.complex128))
    assert out[0] == "OK 0 0 1", out
    rp = np.array([0, 0, 2, 2], np.int64)
    out, dst = run(exe, tmp_path, 3, rp, np.array([0, 2], np.int64), np.array([1.5, 2j]))
    d = read_plan(dst)
    assert out[0].startswith("OK") and not d["real"]
    assert (d["ell_col"][:, 0] == -1).all() and (d["ell_col"][:, 2] == -1).all()


@pytest.mark.parametrize("args,ok,word", [
    ((0, 8, 8, 0, 0, 0, 0), True, ""), ((0, 1, 1, 0, 0, 0, 0), True, ""), ((0, 16, 100, 0, 0, 0, 0), True, ""),
    ((3, 0, 8, 0, 0, 0, 0), False, "truncation"), ((0, 0, 8, 0, 0, 0, 0), False, "restart"), ((0, 17, 8, 0, 0, 0, 0), False, "restart"),
    ((0, 8, 8, 1, 0, 0, 0), False, "preconditioner"), ((0, 8, 8, 0, 1, 0, 0), False, "use_x0"), ((0, 8, 8, 0, 0, 1, 0), False, "flexible"),
    ((0, 8, 8, 0, 0, 0, 1), False, "profile_spmv")])
def test_parameter_refusals(exe, args, ok, word):
    p = subprocess.run([exe, "param"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert lines[0] == ("OK" if ok else "UNSUPPORTED") and word in (lines[1] if len(lines) > 1 else ""), lines
