"""Kernel time per inner step of the fp32 inner solve (C) and of the library's fp64 nested GCR (B), for a kernel trace:

  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python tools/trace_gcr32.py WORKLOAD

applies each inner solver on its own — GCR(8), 8 steps, tol 0, so every step runs — REPS times to the same right-hand side; nothing
else touches the device after set-up.  In the trace the g32_* kernels are C's, every other kernel that ran REPS x the same count is
B's (set-up kernels run once).  Kernel time per inner step = total duration of a side's kernels / (REPS x 8).  WORKLOAD: sample,
poisson, irregular or lattice (tools/bench_gcr32.py's)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, LowPrecisionGCR, Sparse, _lib, problems  # noqa: E402
import bench_gcr32  # noqa: E402

REPS = 5


def main():
    for name, n, rp, ci, va, k, _ in bench_gcr32.workloads([sys.argv[1]]):
        M = Sparse(n, n, rp, ci, va)
        A = M if k is None else DiracOp(M, k)
        ip = GCR_Param(0, 8, 8, 0., False)
        nested, low = GCR(A, ip), LowPrecisionGCR(M, k, ip)
        f, y = Field((n,), problems.rhs_grid(n, 8)), Field((n,))
        for op in (nested, low):
            for _ in range(REPS):
                op(f, y)
            _lib.check(_lib.lib().mgcr_synchronize())
        print(name, "rows", n, "reps", REPS, "inner steps per apply 8; fp32 last:", low.last())


if __name__ == "__main__":
    main()
