"""CPU-side checks of the multi-RHS boundary: every block-of-Fields entry point is declared in include/mgcr.h, exported by
the library and bound in _lib.py; the Python mirror has the classes / methods; nothing computes without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_mvec_create", "mgcr_mvec_destroy", "mgcr_mvec_size", "mgcr_mvec_ncols", "mgcr_mvec_zero", "mgcr_mvec_upload",
       "mgcr_mvec_download", "mgcr_mvec_set_column", "mgcr_mvec_get_column", "mgcr_mvec_dot", "mgcr_mvec_norm2", "mgcr_mvec_axpy",
       "mgcr_op_apply_multi", "mgcr_gcr_solve_multi", "mgcr_bench_op_apply_multi"]


def test_symbols_declared_exported_and_bound():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgcr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgcr_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(L, name), name


def test_python_mirror_has_the_block_interface():
    import mgpreconditionedgcr_amd as m
    assert "MultiField" in m.__all__
    for attr in ("from_fields", "column", "to_numpy", "set_zero", "dot", "squarednorm", "axpy"):
        assert callable(getattr(m.MultiField, attr)), attr
    assert callable(m.Operator.apply_multi) and callable(m.GCR.solve_multi)
    assert callable(m.problems.unstructured_blocks)


def test_no_cpu_fallback_for_blocks():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.mgcr_mvec_create(16, 4, C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
    assert L.mgcr_op_apply_multi(None, None, None) == 2
    assert L.mgcr_gcr_solve_multi(None, None, None, None, None, 0, None, None) == 2
