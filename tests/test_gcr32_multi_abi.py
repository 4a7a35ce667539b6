"""CPU-side checks of the batched low-precision GCR's boundary: the three entry points are declared in include/mgcr.h, exported by
the library and bound in _lib.py with the header's argument counts and types; the header block of its own states Rules M1 and M2, the
lockstep and the freezing, `active`, the launch count, the storage, the counters and every refusal, and the LowPrecisionGCR block
above it still says what it said; the Python and C++ mirrors have the methods; the kernels live in gcr32_multi.hip and the
element-wise expressions in one header that both solves include; nothing is made without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
NEW = ["mgcr_gcr32_apply_multi", "mgcr_gcr32_last_multi", "mgcr_gcr32_solve_multi"]


def header():
    return open(os.path.join(ROOT, "include", "mgcr.h")).read()


def code(path):
    return re.sub(r"//.*", "", open(path).read())


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
    kinds = {"mgcr_op_t": C.c_void_p, "mgcr_mvec_t": C.c_void_p, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double,
             "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double)}
    want = {"mgcr_gcr32_apply_multi": ["mgcr_op_t", "mgcr_mvec_t", "mgcr_mvec_t", "uint32_t"],
            "mgcr_gcr32_last_multi": ["mgcr_op_t", "int32_t *", "double *"],
            "mgcr_gcr32_solve_multi": ["mgcr_op_t", "mgcr_op_t", "double", "int32_t", "int32_t", "mgcr_mvec_t", "mgcr_mvec_t", "double *", "int32_t",
                                       "int32_t *", "int32_t *"]}
    for name in NEW:
        args = [a.strip() for a in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt, flags=re.S).group(1).split(",")]
        types = [re.sub(r"\s+", " ", a if a.endswith("*") else re.sub(r"\s*\w+$", "", a)).replace("* ", "*").strip() for a in args]
        types = [re.sub(r"\s*\*\s*\w*$", " *", t) if "*" in t else t for t in types]
        assert types == want[name], (name, types)
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(sig) == len(types), name
        for t, got in zip(types, sig):
            assert got is kinds[t] or got == kinds[t], (name, t, got)


def test_header_block_of_its_own_states_the_rules():
    txt = header()
    start = txt.index("Batched mixed precision:")
    assert start > txt.index("int mgcr_gcr32_eo_diag")                   # under the LowPrecisionEvenOddGCR block
    doc = txt[start:txt.index("int mgcr_gcr32_apply_multi")]
    for word in ("Rule M1", "Rule M2", "BIT-IDENTICAL", "LOCKSTEP", "share every launch", "frozen", "masked", "`active`", "0 steps and y_j = 0",
                 "Launch count", "4 max_iter + 2", "whatever the data", "nv * k float2", "first batched apply", "stream synchronisation",
                 "mgcr_op_destroy", "gcr32_multi_applies", "gcr32_multi_steps", "do not move", "MGCR_ERR_UNSUPPORTED", "MGCR_ERR_INVALID",
                 "even-odd form", "bits at or above k", "rows != n", "ONE synchronisation", "DEFECT CORRECTION", "hist[j][0] = |r_j| / |b_j|",
                 "never active", "keeps its x", "One\n * synchronisation per outer step", "mgcr_add_scaled(r, b, -1, t)", "mgcr_axpy(1, e, x)",
                 "mgcr_norm2", "MultiDiracOp", "would not contract", "distributed", "GCR or MG objects", "max_outer < 0", "tol < 0",
                 "mgcr_op_apply_multi, mgcr_gcr_solve_multi and\n * the queues go on refusing"):
        assert word in doc, word
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    assert "gcr32_multi_applies" in stat_doc and "gcr32_multi_steps" in stat_doc
    # the LowPrecisionGCR block still refuses the blocks and the queues in its own words
    old = txt[txt.index("LowPrecisionGCR:"):txt.index("int mgcr_gcr32_create")]
    assert "mgcr_mg_create, mgcr_op_apply_multi, mgcr_gcr_solve_multi, mgcr_gcr_solve_queue, mgcr_eo_solve_queue and the storage queries" in old


def test_python_mirror_has_the_methods():
    import mgpreconditionedgcr_amd as m
    cls = m.LowPrecisionGCR
    assert list(inspect.signature(cls.inner_multi).parameters) == ["self", "F", "Y", "active"]
    assert inspect.signature(cls.inner_multi).parameters["Y"].default is None and inspect.signature(cls.inner_multi).parameters["active"].default is None
    assert list(inspect.signature(cls.last_multi).parameters) == ["self"]
    sig = inspect.signature(cls.solve_multi)
    assert list(sig.parameters) == ["self", "A", "B", "X", "tol", "max_outer", "use_x0"]
    assert (sig.parameters["tol"].default, sig.parameters["max_outer"].default, sig.parameters["use_x0"].default) == (1e-10, 50, False)


def test_cpp_mirror_and_example_are_there():
    txt = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    cls = txt[txt.index("class LowPrecisionGCR"):txt.index("class LowPrecisionEvenOddGCR")]
    for word in ("void inner_multi(", "last_multi(", "void solve_multi(", "mgcr_gcr32_apply_multi", "mgcr_gcr32_last_multi", "mgcr_gcr32_solve_multi",
                 "last_history", "last_iterations", "last_converged"):
        assert word in cls, word
    assert os.path.exists(os.path.join(ROOT, "examples", "mixed_precision_batched.cpp"))
    assert "mixed_precision_batched" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_the_kernels_live_in_gcr32_multi_and_the_expressions_in_one_header():
    mk = open(os.path.join(CS, "Makefile")).read()
    assert "gcr32_multi.hip" in mk and "gcr32_elem_dev.h" in mk
    for name in os.listdir(CS):
        if name.endswith((".hip", ".h")) and name != "gcr32_multi.hip":
            assert "__global__" not in "".join(l for l in open(os.path.join(CS, name)) if "g32m_" in l), name
    src = code(os.path.join(CS, "gcr32_multi.hip"))
    assert len(re.findall(r"__global__", src)) == 7                     # entry, apply, dots, build, update, exit, the x correction
    for word in ("atomic", "hipGraph", "hipStreamBeginCapture", "__threadfence", "while (", "asm"):
        assert word not in src, word                                    # no atomics, no capture, no waiting inside a launch
    # one copy of each element-wise expression: defined in the shared headers, in neither .hip file
    elem, row = code(os.path.join(CS, "gcr32_elem_dev.h")), code(os.path.join(CS, "gcr32_row_dev.h"))
    single = code(os.path.join(CS, "gcr32.hip"))
    for fn in ("g32_sub_scaled", "g32_build_dots", "g32_update_one", "norm2d", "fold_betas", "g32_beta_dot"):
        define = r"__device__ __forceinline__ \w+ %s\(" % fn
        assert len(re.findall(define, elem)) == 1, fn
        assert not re.search(define, single) and not re.search(define, src), fn
        assert fn in single and fn in src, fn
    for fn in ("g32_add_product", "g32_dirac_shift", "g32_row_sum", "g32_row_sum_cols"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % fn, row)) == 1, fn
    assert '#include "gcr32_elem_dev.h"' in single and '#include "gcr32_elem_dev.h"' in src
    assert "g32_row_sum_cols<" in src and "g32_row_sum<" in single


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 11.2"):]
    for word in ("Rule M1", "gcr32_multi.hip", "launches per lockstep step", "byte model", "defect correction", "prologue"):
        assert word.lower() in sec.lower(), word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "solve_multi" in readme and "gcr32_multi.hip" in readme


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    assert L.mgcr_gcr32_apply_multi(None, None, None, 0) == 2           # MGCR_ERR_NO_DEVICE
    assert L.mgcr_gcr32_last_multi(None, None, None) == 2
    assert L.mgcr_gcr32_solve_multi(None, None, 1e-10, 5, 0, None, None, None, 0, None, None) == 2
    v = C.c_int64()
    assert L.mgcr_stat(b"gcr32_multi_applies", C.byref(v)) == 0 and v.value == 0
    assert L.mgcr_stat(b"gcr32_multi_steps", C.byref(v)) == 0 and v.value == 0
