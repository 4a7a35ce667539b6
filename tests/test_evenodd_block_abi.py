"""CPU-side checks of the boundary of the even-odd Schur solve with a dense block per site: the three entry points are declared in
include/mgcr.h, exported by the library and bound in _lib.py; the new header block states Rules 1b - 4b and the refusals and leaves
the blocks of mgcr_eo_create and mgcr_eo_create_diag as they were; the Python and C++ mirrors have the two classes; nothing is made
without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_eo_create_block", "mgcr_eo_block_info", "mgcr_eo_block_diag"]


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
    assert len(_lib._SIGS["mgcr_eo_create_block"][1]) == len(_lib._SIGS["mgcr_eo_create_diag"][1]) + 1 == 8


def test_header_block_states_the_rules_and_the_refusals():
    txt = header()
    start = txt.index("int mgcr_eo_diag")
    doc = txt[txt.index("EvenOddBlockDiracOp / EvenOddBlockSparse", start):txt.index("int mgcr_eo_create_block")]
    for word in ("Rule 1b", "Rule 2b", "Rule 3b", "Rule 4b", "Dirac form", "matrix form", "mgcr_eo_block_diag", "mgcr_eo_block_info",
                 "mgcr_eo_half_op", "mgcr_eo_set_k", "mgcr_eo_diag", "MGCR_ERR_INVALID", "MGCR_ERR_UNSUPPORTED", "mgcr_eo_multi_create",
                 "mgcr_eo_solve_queue", "evenodd_block_fused_steps", "stored order", "1 <= bs <= 16", "n % bs", "odd cycle",
                 "differs inside a site", "zero or non-finite pivot", "full-system row of the pivot column", "ONE synchronisation",
                 "the first maximum wins", "Even blocks may be", "would be per column", "ascending"):
        assert word in doc, word
    assert doc.count("BIT-IDENTICAL") == 3
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    assert "evenodd_block_applies" in stat_doc and "evenodd_block_fused_steps" in stat_doc
    # the earlier blocks stay
    old = txt[txt.index("EvenOddDiagDiracOp / EvenOddSparse"):txt.index("int mgcr_eo_create_diag")]
    assert old.count("BIT-IDENTICAL") == 2 and "Rule 1d" in old and "Rule 1b" not in old
    old = txt[txt.index("EvenOddDiracOp:"):txt.index("int mgcr_eo_create")]
    assert "out of scope" in old and old.count("BIT-IDENTICAL") == 2 and "Rule 1b" not in old


def test_python_mirror_has_the_two_classes():
    import mgpreconditionedgcr_amd as m
    for name in ("EvenOddBlockDiracOp", "EvenOddBlockSparse"):
        assert name in m.__all__ and issubclass(getattr(m, name), m.EvenOddDiracOp)
        for method in ("block_diag", "block_info", "set_k", "parity", "sizes", "halves", "split", "merge", "prepare", "reconstruct", "solve"):
            assert callable(getattr(getattr(m, name), method)), (name, method)
    for method in ("split", "merge", "prepare", "reconstruct", "solve", "halves", "set_k"):      # inherited, not re-implemented
        assert getattr(m.EvenOddBlockDiracOp, method) is getattr(m.EvenOddDiracOp, method)
        assert getattr(m.EvenOddBlockSparse, method) is getattr(m.EvenOddDiracOp, method)
    sig = inspect.signature(m.EvenOddBlockDiracOp.__init__)
    assert list(sig.parameters) == ["self", "mat", "k", "bs", "parity"] and sig.parameters["parity"].default is None
    sig = inspect.signature(m.EvenOddBlockSparse.__init__)
    assert list(sig.parameters) == ["self", "mat", "bs", "parity"] and sig.parameters["parity"].default is None
    assert list(inspect.signature(m.EvenOddBlockDiracOp.block_diag).parameters) == ["self"]
    assert list(inspect.signature(m.EvenOddBlockDiracOp.block_info).parameters) == ["self"]
    assert list(inspect.signature(m.EvenOddDiagDiracOp.__init__).parameters) == ["self", "mat", "k", "parity"]


def test_cpp_mirror_and_example_are_there():
    assert '#include "mgcr_dropin.hpp"' in open(os.path.join(ROOT, "include", "mgcr", "Operator.h")).read()     # Operator.h is the drop-in
    txt = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    for word in ("class EvenOddBlockDiracOp", "class EvenOddBlockSparse", "mgcr_eo_create_block", "mgcr_eo_block_diag", "mgcr_eo_block_info"):
        assert word in txt, word
    assert os.path.exists(os.path.join(ROOT, "examples", "clover_evenodd.cpp"))
    assert "clover_evenodd" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_the_new_kernels_live_in_a_file_of_their_own():
    cs = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
    assert "evenodd_block.hip" in open(os.path.join(cs, "Makefile")).read()
    for name in os.listdir(cs):
        if name.endswith(".hip") and name != "evenodd_block.hip":
            assert "__global__" not in "".join(l for l in open(os.path.join(cs, name)) if "blk_" in l), name


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
        assert L.mgcr_eo_create_block(2, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, 2, None, k_arg, C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
        assert not h.value
    out = np.zeros(4, np.complex128)
    assert L.mgcr_eo_block_diag(None, out.ctypes.data, out.ctypes.data) == 2
