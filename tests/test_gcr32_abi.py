"""CPU-side checks of the low-precision GCR's boundary: the six entry points are declared in include/mgcr.h, exported by the library and
bound in _lib.py with the header's argument counts and types; the header block states the arithmetic and the refusals; the Python
and C++ mirrors have the class; the kernels live in a file of their own; nothing is made without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_gcr32_create", "mgcr_gcr32_set_k", "mgcr_gcr32_set_param", "mgcr_gcr32_info", "mgcr_gcr32_apply_matrix", "mgcr_gcr32_last"]


def header():
    return open(os.path.join(ROOT, "include", "mgcr.h")).read()


def test_symbols_declared_exported_and_bound():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(mgcr_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(L, name), name


def test_signatures_match_the_header():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "const int64_t *": C.c_void_p, "const double *": None, "const mgcr_gcr_param *": C.POINTER(_lib.GcrParamC),
             "mgcr_op_t *": C.POINTER(C.c_void_p), "mgcr_op_t": C.c_void_p, "mgcr_vec_t": C.c_void_p, "int64_t *": C.POINTER(C.c_int64),
             "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double)}
    for name in NEW:
        args = [a.strip() for a in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt, flags=re.S).group(1).split(",")]
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(args) == len(sig), (name, args)
        for a, got in zip(args, sig):
            a = re.sub(r"\[2\]$", "", a)
            ctype = re.sub(r"\s*\w+$", "", a).strip() if not a.endswith("*") else a
            ctype = re.sub(r"\s+", " ", ctype).replace(" *", " *")
            if re.search(r"\w+\[2\]$", a.replace(" ", "")) or a.startswith("const double"):
                assert got in (C.POINTER(C.c_double), C.c_void_p), (name, a)      # arrays of doubles: a pointer either way
                continue
            want = kinds[ctype]
            assert got is want or got == want, (name, a, got)


def test_header_block_states_the_arithmetic_and_the_refusals():
    txt = header()
    doc = txt[txt.index("LowPrecisionGCR:"):txt.index("int mgcr_gcr32_create")]
    for word in ("float2", "round to nearest", "k32 = (float)k", "nothing is fused", "stored order", "second accumulator", "y = x - k32 s",
                 "converted to double", "fixed order", "no atomics", "bit-reproducible", "rounded to float once", "restarted GCR",
                 "beta_j = <Ap_j, Ap> / <Ap_j, Ap_j>", "alpha = <Ap, r> / <Ap, Ap>", "wiped every `restart` steps", "never NaN", "x0 = 0",
                 "MGCR_ERR_UNSUPPORTED", "MGCR_ERR_INVALID", "restart > 16", "use_x0", "profile_spmv", "names the row", "flexible = 1",
                 "not a linear map", "left_precond", "mgcr_mg_create", "mgcr_op_apply_multi", "mgcr_gcr_solve_multi", "mgcr_gcr_solve_queue",
                 "mgcr_eo_solve_queue", "distributed", "gcr32_applies", "gcr32_steps", "mgcr_op_destroy"):
        assert word in doc, word
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    assert "gcr32_applies" in stat_doc and "gcr32_steps" in stat_doc
    assert "ONE synchronisation" in txt[txt.index("int mgcr_gcr32_apply_matrix"):txt.index("int mgcr_gcr32_last")]


def test_python_mirror_has_the_class():
    import mgpreconditionedgcr_amd as m
    assert "LowPrecisionGCR" in m.__all__ and issubclass(m.LowPrecisionGCR, m.api.Operator)
    for method in ("set_k", "set_param", "apply_matrix", "last", "info"):
        assert callable(getattr(m.LowPrecisionGCR, method)), method
    sig = inspect.signature(m.LowPrecisionGCR.__init__)
    assert list(sig.parameters) == ["self", "mat", "k", "gcr_param"] and sig.parameters["k"].default is None
    p = m.GCR_Param(0, 5, 100, 1e-10, False, solver_r=None, flexible=True)
    assert p.flexible and p._c().flexible == 1


def test_cpp_mirror_and_example_are_there():
    txt = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    for word in ("class LowPrecisionGCR", "mgcr_gcr32_create", "mgcr_gcr32_set_k", "mgcr_gcr32_apply_matrix", "mgcr_gcr32_last", "mgcr_gcr32_info"):
        assert word in txt, word
    assert '#include "mgcr_dropin.hpp"' in open(os.path.join(ROOT, "include", "mgcr", "GCR.h")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "mixed_precision.cpp"))
    assert "mixed_precision" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_the_new_kernels_live_in_a_file_of_their_own():
    cs = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    assert "gcr32.hip" in mk and "gcr32_plan.h" in mk
    for name in os.listdir(cs):
        if name.endswith(".hip") and name != "gcr32.hip":
            assert "__global__" not in "".join(l for l in open(os.path.join(cs, name)) if "g32_" in l), name
    plan = open(os.path.join(cs, "gcr32_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", plan)                       # pure host code
    src = open(os.path.join(cs, "gcr32.hip")).read()
    for word in ("atomic", "hipGraph", "hipStreamBeginCapture", "__threadfence", "while (", "asm"):
        assert word not in re.sub(r"//.*", "", src), word              # no atomics, no capture, no waiting inside a launch


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 11."):]
    for word in ("byte model", "fp32", "gcr32", "follow-ups", "stencil", "half-precision"):
        assert word.lower() in sec.lower(), word
    assert "LowPrecisionGCR" in open(os.path.join(ROOT, "README.md")).read()
    assert "right_precond_solver" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    rowptr = np.array([0, 2, 4], np.int64)
    col = np.array([0, 1, 0, 1], np.int64)
    val = np.array([2.0, -1.0, -1.0, 2.0], np.complex128)
    k = (C.c_double * 2)(0.1, 0.0)
    pc = _lib.GcrParamC(0, 8, 8, 0.1, 0, None, None, 0, 0, 0, 0)
    for k_arg in (k, None):
        h = C.c_void_p()
        assert L.mgcr_gcr32_create(2, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, k_arg, C.byref(pc), C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
        assert not h.value
    assert L.mgcr_gcr32_last(None, None, None) == 2
    assert L.mgcr_gcr32_apply_matrix(None, None, None) == 2
    # ... and what needs no device: handles that are not a low-precision GCR
    assert L.mgcr_gcr32_set_k(None, k) == 1 and L.mgcr_gcr32_set_param(None, C.byref(pc)) == 1
    assert L.mgcr_gcr32_info(None, None, None, None, None, None) == 1
    v = C.c_int64()
    assert L.mgcr_stat(b"gcr32_applies", C.byref(v)) == 0 and v.value == 0
    assert L.mgcr_stat(b"gcr32_steps", C.byref(v)) == 0 and v.value == 0
