"""CPU-side checks of the queued even-odd scan's boundary: mgcr_eo_solve_queue is declared in include/mgcr.h with the argument list
the issue fixed, exported by the cross-compiled library and bound in _lib.py with matching types; the header states the per-system
rule and the counters; the Python and C++ mirrors have the method; nothing runs without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgcr_eo_solve_queue"
ARGS = [("mgcr_op_t", "eo"), ("const mgcr_gcr_param *", "param"), ("int32_t", "width"), ("int32_t", "nsys"), ("const mgcr_vec_t *", "rhs_full"),
        ("const mgcr_vec_t *", "x_full"), ("const double *", "k_ri"), ("double *", "hist"), ("int32_t", "hist_cap"), ("int32_t *", "n_iter"),
        ("int32_t *", "converged")]


def test_symbol_declared_exported_and_bound():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgcr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgcr_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    assert NAME in declared
    assert NAME in _lib.exported_symbols()
    assert hasattr(L, NAME)
    m = re.search(r"int mgcr_eo_solve_queue\((.*?)\);", txt, re.S)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    got = [(a[:len(a) - len(a.split()[-1].lstrip("*"))].strip(), a.split()[-1].lstrip("*")) for a in args]
    assert got == ARGS, got
    restype, argtypes = _lib._SIGS[NAME]
    vp = C.c_void_p
    assert restype is C.c_int
    assert len(argtypes) == len(ARGS)
    assert argtypes[0] is vp and argtypes[2] is C.c_int32 and argtypes[3] is C.c_int32 and argtypes[8] is C.c_int32
    assert argtypes[1] is C.POINTER(_lib.GcrParamC)
    assert argtypes[4] is C.POINTER(vp) and argtypes[5] is C.POINTER(vp)
    assert argtypes[6] is C.POINTER(C.c_double)
    assert argtypes[9] is C.POINTER(C.c_int32) and argtypes[10] is C.POINTER(C.c_int32)
    assert _lib._SIGS[NAME] == _lib._SIGS["mgcr_gcr_solve_queue"]       # the queue's argument list, with eo and full Fields


def test_header_states_the_rule_and_the_counters():
    txt = open(os.path.join(ROOT, "include", "mgcr.h")).read()
    doc = txt[txt.index("Queued even-odd scan"):txt.index("int mgcr_eo_solve_queue")]
    assert "BIT-IDENTICAL to mgcr_eo_solve" in doc and "EvenOddDiracOp(D, k_s)" in doc
    for word in ("check_every", "pairwise", "use_x0", "MGCR_ERR_INVALID", "MGCR_ERR_UNSUPPORTED", "n_e", "mgcr_finalize"):
        assert word in doc, word
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    for counter in ("eo_queue_solves", "eo_queue_admissions", "eo_queue_steps"):
        assert counter in stat_doc and counter in doc, counter
    multi_doc = txt[txt.index("int mgcr_eo_multi_create") - 3000:txt.index("int mgcr_eo_multi_create")]
    assert "Out of scope: distributed halves" in multi_doc and "mgcr_eo_solve_queue" in multi_doc


def test_mirrors_have_the_method():
    import mgpreconditionedgcr_amd as m
    sig = inspect.signature(m.EvenOddDiracOp.solve_queue)
    assert list(sig.parameters) == ["self", "rhs_list", "x_list", "ks", "gcr_param", "width"]
    assert sig.parameters["width"].default == 8
    ref = inspect.signature(m.experiments.test_kcritical_evenodd).parameters
    got = inspect.signature(m.experiments.test_kcritical_evenodd_queue).parameters
    assert list(got) == list(ref) + ["width"] and got["width"].default == 4
    assert all(got[n].default == ref[n].default for n in ref)
    hpp = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    assert re.search(r"void solve_queue\(const std::vector<const Field<num_type> \*> &\w+, const std::vector<Field<num_type> \*> &\w+, "
                     r"const std::vector<std::complex<double>> &\w+,\s*GCR_Param<num_type> \*\w+, int width = 8\)", hpp)
    assert "mgcr_eo_solve_queue(" in hpp


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    assert L.mgcr_eo_solve_queue(None, None, 2, 1, None, None, None, None, 0, None, None) == 2  # MGCR_ERR_NO_DEVICE
    v = C.c_int64(-1)
    for name in (b"eo_queue_solves", b"eo_queue_admissions", b"eo_queue_steps"):
        assert L.mgcr_stat(name, C.byref(v)) == 0 and v.value == 0
