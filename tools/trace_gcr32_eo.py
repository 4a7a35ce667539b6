"""Kernel time per inner Schur step of the fp32 inner solve on the even-odd Schur system (side E of tools/bench_gcr32_eo.py) and of
the library's fp64 GCR on the same Schur operator (side D's step), for a kernel trace:

  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python tools/trace_gcr32_eo.py WORKLOAD

applies each solver on its own — GCR(8), 8 steps, tol 0, so every step runs — REPS times to the same right-hand side on the even
half; nothing else touches the device after set-up.  In the trace the g32_* kernels are the fp32 side's (g32_eo_stage1_kernel and
g32_eo_stage2_kernel its matrix apply), every other kernel of the library whose call count is a multiple of REPS is the fp64 side's
(set-up kernels run once or three times).  Kernel time per inner step = total duration of a side's kernels / (REPS x 8).  WORKLOAD: sample, lattice, twisted or poisson
(tools/bench_gcr32_eo.py's).

  python tools/trace_gcr32_eo.py --summarise NAME_kernel_stats.csv   prints the two sums as JSON"""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS = 5
STEPS = 8


def summarise(path):
    """kernel_stats.csv -> per-step kernel times: the g32_ kernels by name, the library's other kernels whose call count is a multiple
    of REPS (the fp64 side: its step kernels and the few per-apply ones, all divided by the steps)"""
    fp32, fp64 = {}, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, calls, total = row["Name"], int(row["Calls"]), float(row["TotalDurationNs"])
            short = name.split("(")[0].replace("void mgcr::", "")
            if "g32_" in name:
                fp32[short] = fp32.get(short, 0.) + total
            elif calls % REPS == 0 and "mgcr::" in name:   # (a step kernel templated on the stored directions runs REPS times per form)
                fp64[short] = fp64.get(short, 0.) + total
    per = 1e-3 / (REPS * STEPS)
    step32 = sum(v for k, v in fp32.items() if "entry" not in k and "exit" not in k)
    return {"fp32_step_us": step32 * per, "fp32_apply_us": sum(v for k, v in fp32.items() if "g32_eo_stage" in k) * per,
            "fp32_stage1_us": sum(v for k, v in fp32.items() if "stage1" in k) * per,
            "fp32_stage2_us": sum(v for k, v in fp32.items() if "stage2" in k) * per,
            "fp32_entry_exit_us_per_apply": sum(v for k, v in fp32.items() if "entry" in k or "exit" in k) * 1e-3 / REPS,
            "fp64_step_us": sum(fp64.values()) * per, "fp64_kernels_us_per_step": {k: v * per for k, v in sorted(fp64.items())}}


def main():
    if sys.argv[1] == "--summarise":
        print(json.dumps(summarise(sys.argv[2]), indent=1, sort_keys=True))
        return
    from mgpreconditionedgcr_amd import EvenOddDiagDiracOp, EvenOddSparse, Field, GCR, GCR_Param, LowPrecisionEvenOddGCR, Sparse, _lib, problems
    import bench_gcr32_eo
    for name, n, rp, ci, va, k, _ in bench_gcr32_eo.workloads([sys.argv[1]]):
        M = Sparse(n, n, rp, ci, va)
        S = EvenOddSparse(M) if k is None else EvenOddDiagDiracOp(M, k)
        ip = GCR_Param(0, 8, STEPS, 0., False)
        nested, low = GCR(S, ip), LowPrecisionEvenOddGCR(M, k, ip)
        ne = S.sizes()[1]
        f, y = Field((ne,), problems.rhs_grid(ne, 8)), Field((ne,))
        for op in (nested, low):
            for _ in range(REPS):
                op(f, y)
            _lib.check(_lib.lib().mgcr_synchronize())
        print(name, "even rows", ne, "reps", REPS, "inner steps per apply", STEPS, "; fp32 last:", low.last())


if __name__ == "__main__":
    main()
