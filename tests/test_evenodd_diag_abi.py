"""CPU-side checks of the boundary of the even-odd Schur solve with a site diagonal: the two entry points are declared in
include/mgcr.h, exported by the library and bound in _lib.py; the new header block states Rules 1d - 3d and the refused entry points,
and leaves the block of mgcr_eo_create as it was; the Python mirror has the two classes; nothing is made without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_eo_create_diag", "mgcr_eo_diag"]


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


def test_argument_counts_match_the_header():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt, flags=re.S).group(1).split(",")
        assert len(args) == len(_lib._SIGS[name][1]), (name, args)
    assert len(_lib._SIGS["mgcr_eo_create_diag"][1]) == len(_lib._SIGS["mgcr_eo_create"][1]) == 7


def test_header_block_states_the_rules_and_the_refusals():
    txt = header()
    start = txt.index("int mgcr_eo_reconstruct")
    doc = txt[txt.index("EvenOddDiagDiracOp / EvenOddSparse", start):txt.index("int mgcr_eo_create_diag")]
    for word in ("Rule 1d", "Rule 2d", "Rule 3d", "Dirac form", "matrix form", "mgcr_eo_diag", "mgcr_eo_half_op", "mgcr_eo_set_k",
                 "MGCR_ERR_INVALID", "MGCR_ERR_UNSUPPORTED", "mgcr_eo_multi_create", "mgcr_eo_solve_queue", "evenodd_diag_fused_steps",
                 "names the full-system row", "stored order"):
        assert word in doc, word
    assert doc.count("BIT-IDENTICAL") == 2
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    assert "evenodd_diag_fused_steps" in stat_doc and "evenodd_fused_steps" in stat_doc
    # the block of mgcr_eo_create stays: a diagonal is still out of ITS scope
    old = txt[txt.index("EvenOddDiracOp:"):txt.index("int mgcr_eo_create")]
    assert "diagonal" in old and "out of scope" in old and old.count("BIT-IDENTICAL") == 2 and "Rule 1d" not in old


def test_python_mirror_has_the_two_classes():
    import mgpreconditionedgcr_amd as m
    for name in ("EvenOddDiagDiracOp", "EvenOddSparse"):
        assert name in m.__all__ and issubclass(getattr(m, name), m.EvenOddDiracOp)
        for method in ("diag", "set_k", "parity", "sizes", "halves", "split", "merge", "prepare", "reconstruct", "solve"):
            assert callable(getattr(getattr(m, name), method)), (name, method)
    for method in ("split", "merge", "prepare", "reconstruct", "solve", "halves"):           # inherited, not re-implemented
        assert getattr(m.EvenOddDiagDiracOp, method) is getattr(m.EvenOddDiracOp, method)
        assert getattr(m.EvenOddSparse, method) is getattr(m.EvenOddDiracOp, method)
    sig = inspect.signature(m.EvenOddDiagDiracOp.__init__)
    assert list(sig.parameters) == ["self", "mat", "k", "parity"] and sig.parameters["parity"].default is None
    sig = inspect.signature(m.EvenOddSparse.__init__)
    assert list(sig.parameters) == ["self", "mat", "parity"] and sig.parameters["parity"].default is None
    assert list(inspect.signature(m.EvenOddDiagDiracOp.diag).parameters) == ["self"]
    assert list(inspect.signature(m.EvenOddDiracOp.__init__).parameters) == ["self", "mat", "k", "parity"]


def test_cpp_mirror_and_example_are_there():
    assert '#include "mgcr_dropin.hpp"' in open(os.path.join(ROOT, "include", "mgcr", "Operator.h")).read()     # Operator.h is the drop-in
    txt = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    assert "class EvenOddDiagDiracOp" in txt and "class EvenOddSparse" in txt and "mgcr_eo_create_diag" in txt and "mgcr_eo_diag" in txt
    assert os.path.exists(os.path.join(ROOT, "examples", "poisson_evenodd.cpp"))
    assert "poisson_evenodd" in open(os.path.join(ROOT, "examples", "Makefile")).read()


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
    for k_arg in (k, None):
        h = C.c_void_p()
        assert L.mgcr_eo_create_diag(2, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, None, k_arg, C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
        assert not h.value
    out = np.zeros(2, np.complex128)
    assert L.mgcr_eo_diag(None, out.ctypes.data, out.ctypes.data) == 2
