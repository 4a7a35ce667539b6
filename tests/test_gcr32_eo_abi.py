"""CPU-side checks of the even-odd low-precision GCR's boundary: the three entry points are declared in include/mgcr.h, exported by
the library and bound in _lib.py with the header's argument counts and types; the header block states the arithmetic and the
refusals; the Python and C++ mirrors have the class; the kernels live in a file of their own and gcr32.hip keeps its one row sum in a
header both include; nothing is made without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_gcr32_create_eo", "mgcr_gcr32_eo_info", "mgcr_gcr32_eo_diag"]


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
    kinds = {"int64_t": (C.c_int64,), "const int64_t *": (C.c_void_p,), "const double *": (C.POINTER(C.c_double), C.c_void_p),
             "const int8_t *": (C.c_void_p,), "float *": (C.c_void_p,), "const mgcr_gcr_param *": (C.POINTER(_lib.GcrParamC),),
             "mgcr_op_t *": (C.POINTER(C.c_void_p),), "mgcr_op_t": (C.c_void_p,), "int64_t *": (C.POINTER(C.c_int64),),
             "int32_t *": (C.POINTER(C.c_int32),)}
    for name in NEW:
        args = [a.strip() for a in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt, flags=re.S).group(1).split(",")]
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(args) == len(sig), (name, args)
        for a, got in zip(args, sig):
            ctype = re.sub(r"\s+", " ", re.sub(r"\w+$", "", a)).strip()
            assert any(got is w or got == w for w in kinds[ctype]), (name, a, got)


def test_header_block_states_the_arithmetic_and_the_refusals():
    txt = header()
    doc = txt[txt.index("LowPrecisionEvenOddGCR:"):txt.index("int mgcr_gcr32_create_eo")]
    for word in ("S = diag(a_e) - c^2 H_eo diag(1 / a_o) H_oe", "dim = nrow = n_e", "mgcr_eo_create_diag", "mgcr_eo_create_block", "(float)re, (float)im",
                 "bit for bit", "c2_32 = (float) of c c", "un-fused", "one flag", "u = H_oe32 r", "t = inv_o32 (.) u", "v = H_eo32 t", "w = c2_32 v",
                 "y = a_e32 (.) r - w", "y = r - w", "4 max_iter + 2", "n_o elements", "MGCR_ERR_INVALID", "MGCR_ERR_UNSUPPORTED", "parity vector",
                 "k is NOT compared", "site blocks", "full-system row", "leaves the operator as it was", "mgcr_gcr32_eo_info", "flexible = 1",
                 "refuse any preconditioner"):
        assert word in doc, word


def test_python_mirror_has_the_class():
    import mgpreconditionedgcr_amd as m
    assert "LowPrecisionEvenOddGCR" in m.__all__ and issubclass(m.LowPrecisionEvenOddGCR, m.LowPrecisionGCR)
    for method in ("set_k", "set_param", "apply_matrix", "last", "info", "diag", "sizes"):
        assert callable(getattr(m.LowPrecisionEvenOddGCR, method)), method
    sig = inspect.signature(m.LowPrecisionEvenOddGCR.__init__)
    assert list(sig.parameters) == ["self", "mat", "k", "gcr_param", "parity"]
    assert all(sig.parameters[p].default is None for p in ("k", "gcr_param", "parity"))


def test_cpp_mirror_and_example_are_there():
    txt = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    for word in ("class LowPrecisionEvenOddGCR : public LowPrecisionGCR<num_type>", "mgcr_gcr32_create_eo", "mgcr_gcr32_eo_info", "mgcr_gcr32_eo_diag"):
        assert word in txt, word
    assert os.path.exists(os.path.join(ROOT, "examples", "mixed_precision_evenodd.cpp"))
    assert "mixed_precision_evenodd" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def code_only(path):
    return re.sub(r"//.*", "", open(path).read())


def test_the_new_kernels_live_in_a_file_of_their_own_and_share_the_row_sum():
    cs = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    for f in ("gcr32_eo.hip", "gcr32_eo_plan.h", "gcr32_state.h", "gcr32_row_dev.h"):
        assert f in mk, f
    src, base = code_only(os.path.join(cs, "gcr32_eo.hip")), code_only(os.path.join(cs, "gcr32.hip"))
    assert "g32_eo_stage1_kernel" in src and "g32_eo_stage2_kernel" in src and "g32_eo_" not in base.replace("gcr32_eo_", "")
    # one copy of the row sum: defined in the device header, called by the three kernels, written out in neither .hip
    row = code_only(os.path.join(cs, "gcr32_row_dev.h"))
    assert row.count("void g32_row_sum(") == 1
    assert base.count("g32_row_sum<REAL>(") == 1 and src.count("g32_row_sum<REAL>(") == 2
    for text in (src, base):
        assert "tail_ptr[t" not in text and "A.col[" not in text
    plan = code_only(os.path.join(cs, "gcr32_eo_plan.h"))
    assert "hip" not in plan                                            # pure host code
    for word in ("atomic", "hipGraph", "hipStreamBeginCapture", "__threadfence", "while (", "asm"):
        assert word not in src, word                                    # no atomics, no capture, no waiting inside a launch


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 11."):]
    for word in ("gcr32_eo", "g32_eo_stage1_kernel", "g32_eo_stage2_kernel", "4 · max_iter + 2", "Follow-ups", "mgcr_gcr32_create_eo"):
        assert word in sec, word
    assert "LowPrecisionEvenOddGCR" in open(os.path.join(ROOT, "README.md")).read()


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    rowptr = np.array([0, 1, 2], np.int64)
    col = np.array([1, 0], np.int64)
    val = np.array([-1.0, -1.0], np.complex128)
    k = (C.c_double * 2)(0.1, 0.0)
    pc = _lib.GcrParamC(0, 8, 8, 0.1, 0, None, None, 0, 0, 0, 0)
    for k_arg in (k, None):
        h = C.c_void_p()
        assert L.mgcr_gcr32_create_eo(2, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, None, k_arg, C.byref(pc), C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
        assert not h.value
    assert L.mgcr_gcr32_eo_diag(None, None, None) == 2
    # ... and what needs no device: a handle that is not a low-precision GCR in even-odd form
    assert L.mgcr_gcr32_eo_info(None, *([None] * 10)) == 1
