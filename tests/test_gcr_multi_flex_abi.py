"""CPU-side checks of the flexible batched GCR's boundary: the header block of its own under mgcr_gcr_solve_multi states the slot kinds,
Rule F, the gate and the mask, the storage, the launch count, the counters and every refusal, and the blocks around it still say what
they said; the counter answers without a GPU; the Python and C++ mirrors' docstrings name the feature and the example is there; the new
kernels live in csrc/gcr_multi_flex.hip under names of their own — gcr32_multi.hip still has its seven __global__ functions and
gcr_multi.hip defines no new one; the documents record it."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")


def header():
    return open(os.path.join(ROOT, "include", "mgcr.h")).read()


def code(path):
    return re.sub(r"//.*", "", open(path).read())


def test_header_block_of_its_own_states_the_rules():
    txt = header()
    start = txt.index("Flexible batched GCR:")
    assert txt.index("k independent solves A x_j = rhs_j") < start < txt.index("int mgcr_gcr_solve_multi")      # under mgcr_gcr_solve_multi
    doc = txt[start:txt.index("int mgcr_gcr_solve_multi")]
    for word in ("param->flexible == 1", "right_precond", "(a) a LowPrecisionGCR of the square form", "LOCKSTEP", "(b) any operator that mgcr_op_apply_multi takes",
                 "Sparse, DiracOp, HierarchicalSparse", "a preconditioner at another k is legitimate", "MultiDiracOp",
                 "Rule F", "BIT-IDENTICAL", "mgcr_gcr_solve(A_j, param, rhs_j)", "A_j = DiracOp(D, ks[j])", "whatever the other columns do",
                 "mgcr_op_xr_fuse_kind 0 or 1", "gcr_small_eligible", "never takes the one-workgroup path", "at every n",
                 "The mask", "FROZEN", "pending", "still active", "The gate", "stopping test", "0 steps", "D = 0", "mgcr_gcr32_last_multi",
                 "Launches per outer step", "whatever the data", "4 m + 2 - ceil(m / restart_inner)", "plus 1, the gate", "No host round trip",
                 "check_every", "exactly the launches it enqueued before", "Storage: one more n x k block", "allocated only by a flexible solve",
                 "multi_flex_solves", "gcr32_multi_applies", "gcr32_multi_steps",
                 "MGCR_ERR_UNSUPPORTED", "a left preconditioner", "flexible == 0", "GCR or MG object", "even-odd `low`", "a low-precision GCR as A",
                 "profile_spmv", "distributed operators", "truncation or full", "cycles longer than 16", "MGCR_ERR_INVALID", "dimension is not n",
                 "Nothing is\n * written to x in any refused call", "mgcr_eo_multi_solve, mgcr_gcr_solve_queue and mgcr_eo_solve_queue go on refusing"):
        assert word in doc, word
    # the unpreconditioned block above it keeps its words, qualified
    old = txt[txt.index("k independent solves A x_j = rhs_j"):start]
    for word in ("unpreconditioned", "a left or\n * right preconditioner, flexible", "BIT-IDENTICAL to mgcr_gcr_solve(A, param, rhs_j)",
                 "2 + 2 * min(restart, max_iter + 1) blocks of n x k"):
        assert word in old, word
    # the sentences other blocks are held to
    assert "The batched and queued solves refuse any preconditioner" in txt
    assert "mgcr_op_apply_multi, mgcr_gcr_solve_multi and\n * the queues go on refusing" in txt
    assert "mgcr_mg_create, mgcr_op_apply_multi, mgcr_gcr_solve_multi, mgcr_gcr_solve_queue, mgcr_eo_solve_queue and the storage queries" in txt
    stat_doc = txt[txt.index("Counters for tests and benchmarks"):txt.index("int mgcr_stat")]
    assert '"multi_flex_solves" = flexible batched solves' in stat_doc


def test_the_counter_answers_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mgpreconditionedgcr_amd import _lib
    L = _lib.lib()
    v = C.c_int64(-1)
    assert L.mgcr_stat(b"multi_flex_solves", C.byref(v)) == 0 and v.value == 0
    assert L.mgcr_gcr_solve_multi(None, None, None, None, None, 0, None, None) == 2          # MGCR_ERR_NO_DEVICE: no CPU fallback


def test_the_counter_is_wired():
    api = code(os.path.join(CS, "api.hip"))
    assert '"multi_flex_solves"' in api and "gcr_multi_flex_solve_count()" in api
    assert "g_multi_flex_solves++" in code(os.path.join(CS, "gcr_multi.hip"))


def test_python_and_cpp_mirrors_and_the_example():
    import mgpreconditionedgcr_amd as m
    doc = m.GCR.solve_multi.__doc__
    for word in ("flexible", "solver_r=M", "LowPrecisionGCR", "Rule F", "Sparse, DiracOp, HierarchicalSparse"):
        assert word in doc, word
    src = open(os.path.join(ROOT, "mgpreconditionedgcr_amd", "api.py")).read()
    at = src.index("    def solve_multi(self, RHS, X):")
    body = src[at:src.index("    def solve_queue(", at)]
    assert "self._keep.append(self.param.right_precond)" in body                              # keeps its preconditioner alive
    hpp = open(os.path.join(ROOT, "include", "mgcr", "mgcr_dropin.hpp")).read()
    cls = hpp[hpp.index("    // k independent solves A x_j = rhs_j in lockstep"):hpp.index("    void solve_multi(const MultiField<num_type> &rhs")]
    for word in ("flexible = true", "right_precond = M", "LowPrecisionGCR", "Rule F"):
        assert word in cls, word
    ex = os.path.join(ROOT, "examples", "mixed_precision_batched_flexible.cpp")
    assert os.path.exists(ex)
    text = open(ex).read()
    assert "mixed.solve_multi(B, X)" in text and "outer.flexible = true" in text and "double k = 0.18" in text and "ncols = 4" in text
    assert "mixed_precision_batched_flexible" in open(os.path.join(ROOT, "examples", "Makefile")).read()


def test_the_kernels_live_in_a_file_of_their_own():
    mk = open(os.path.join(CS, "Makefile")).read()
    assert "gcr_multi_flex.hip" in mk
    flex = code(os.path.join(CS, "gcr_multi_flex.hip"))
    names = re.findall(r"__global__ void (?:__launch_bounds__\([^)]*\) )?(\w+)\(", flex)
    assert sorted(names) == ["mflex_exit_kernel", "mflex_gate_kernel", "mflex_take_kernel"]
    for word in ("atomic", "hipGraph", "hipStreamBeginCapture", "__threadfence", "while (", "asm"):
        assert word not in flex, word                                    # no atomics, no capture, no waiting inside a launch
    assert "g32m_" not in "".join(l for l in flex.splitlines() if "__global__" in l)
    # gcr32_multi.hip: host code only was added
    g32 = code(os.path.join(CS, "gcr32_multi.hip"))
    assert len(re.findall(r"__global__", g32)) == 7
    assert "mflex_gate(" in g32 and "mflex_exit(" in g32 and "MFlexGate" in g32
    # gcr_multi.hip: the kernels it had, and no other
    multi = code(os.path.join(CS, "gcr_multi.hip"))
    kernels = sorted(set(re.findall(r"\b([mq]_\w+_kernel)\b", "\n".join(l for l in multi.splitlines() if "__global__" in l or "__launch_bounds__" in l))))
    assert kernels == ["m_alpha_kernel", "m_build_kernel", "m_close_x_kernel", "m_coef_kernel", "m_dot_kernel", "m_finish_kernel", "m_init_kernel",
                       "m_init_partials_kernel", "m_pending_x_kernel", "m_reset_kernel", "m_resid_sub_kernel", "m_xr_kernel", "q_admit_state_kernel",
                       "q_r0_kernel", "q_scatter_kernel"]
    assert len(re.findall(r"__global__", multi)) == 15
    assert "mflex_" not in "".join(l for l in multi.splitlines() if "__global__" in l)
    ih = code(os.path.join(CS, "internal.h"))
    assert "struct MFlexGate" in ih and ih.index("struct Gcr32Gate") < ih.index("struct MFlexGate")


def test_documents_name_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 11.3"):]
    for word in ("Rule F", "gcr_multi_flex.hip", "mflex_gate_kernel", "mflex_exit", "mflex_take", "one more launch per outer step",
                 "frozen", "pending", "defect correction", "when to use"):
        assert word.lower() in sec.lower(), word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "gcr_multi_flex.hip" in readme and "flexible=True" in readme
