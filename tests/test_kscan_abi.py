"""CPU-side checks of the hopping-parameter scan's boundary: the two MultiDiracOp entry points are declared in include/mgcr.h,
exported by the library and bound in _lib.py; the Python mirror has the class and the batched experiment; nothing is made
without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgcr_dirac_multi_create", "mgcr_dirac_multi_set_k"]


def test_symbols_declared_exported_and_bound():
    from mgpreconditionedgcr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgcr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgcr_[a-z0-9_]+)\s*\(", txt))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(L, name), name


def test_header_states_the_two_rules():
    txt = open(os.path.join(ROOT, "include", "mgcr.h")).read()
    doc = txt[txt.index("MultiDiracOp:"):txt.index("int mgcr_dirac_multi_create")]
    assert "Rule 1" in doc and "Rule 2" in doc and doc.count("BIT-IDENTICAL") == 2


def test_python_mirror_has_the_scan_interface():
    import mgpreconditionedgcr_amd as m
    assert "MultiDiracOp" in m.__all__ and issubclass(m.MultiDiracOp, m.Operator)
    assert callable(m.MultiDiracOp.set_k)
    sig = inspect.signature(m.experiments.test_kcritical_batched)
    assert list(sig.parameters) == list(inspect.signature(m.experiments.test_kcritical).parameters)
    assert {n: p.default for n, p in sig.parameters.items() if p.default is not p.empty} == \
        dict(steps=5, restart=10, max_iter=50000, tol=1e-13, seed=42)


def test_no_cpu_fallback_for_the_scan_operator():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    ks = (C.c_double * 4)(0.1, 0.0, 0.2, 0.0)
    assert L.mgcr_dirac_multi_create(None, 2, ks, C.byref(h)) == 2  # MGCR_ERR_NO_DEVICE
    assert not h.value
