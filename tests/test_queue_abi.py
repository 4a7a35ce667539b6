"""CPU-side checks of the queued batched GCR's boundary: mgcr_gcr_solve_queue is declared in include/mgcr.h, exported by the library and
bound in _lib.py; the header states the per-system rule; the Python and C++ mirrors have the method; nothing runs without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgcr_gcr_solve_queue"


def test_symbol_declared_exported_and_bound():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgcr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgcr_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    assert NAME in declared
    assert NAME in _lib.exported_symbols()
    assert hasattr(L, NAME)
    m = re.search(r"int mgcr_gcr_solve_queue\((.*?)\);", txt, re.S)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 11 == len(_lib._SIGS[NAME][1]), args
    assert [a.split()[-1].lstrip("*") for a in args] == ["A", "param", "width", "nsys", "rhs", "x", "k_ri", "hist", "hist_cap", "n_iter", "converged"]


def test_header_states_the_per_system_rule():
    txt = open(os.path.join(ROOT, "include", "mgcr.h")).read()
    doc = txt[txt.index("Queued batched GCR"):txt.index("int mgcr_gcr_solve_queue")]
    assert "BIT-IDENTICAL to mgcr_gcr_solve on that system alone" in doc
    assert "DiracOp(D, k_s)" in doc and "check_every" in doc and "pairwise" in doc
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    for counter in ("queue_solves", "queue_admissions", "queue_steps"):
        assert counter in stat_doc, counter


def test_mirrors_have_the_method():
    import mgpreconditionedgcr_amd as m
    sig = inspect.signature(m.GCR.solve_queue)
    assert list(sig.parameters) == ["self", "rhs_list", "x_list", "width", "ks"]
    assert sig.parameters["width"].default == 8 and sig.parameters["ks"].default is None
    ref = inspect.signature(m.experiments.test_kcritical).parameters
    got = inspect.signature(m.experiments.test_kcritical_queue).parameters
    assert list(got) == list(ref) + ["width"] and got["width"].default == 4
    assert all(got[n].default == ref[n].default for n in ref)
    hpp = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    assert re.search(r"void solve_queue\(const std::vector<const Field<num_type> \*> &\w+, const std::vector<Field<num_type> \*> &\w+, int width,\s*"
                     r"const std::vector<std::complex<double>> \*ks = nullptr\)", hpp)
    assert "mgcr_gcr_solve_queue(" in hpp


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    assert L.mgcr_gcr_solve_queue(None, None, 2, 1, None, None, None, None, 0, None, None) == 2  # MGCR_ERR_NO_DEVICE
    v = C.c_int64(-1)
    assert L.mgcr_stat(b"queue_steps", C.byref(v)) == 0 and v.value == 0
