"""Kernel time of one OUTER step of the flexible batched GCR, for a kernel trace: the gate, the masked exit (and, for another
preconditioner than a low-precision GCR, the masked copy) beside the lockstep inner steps and the batched outer kernels.

  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python tools/trace_gcr_multi_flex.py run WORKLOAD WIDTH
  python tools/trace_gcr_multi_flex.py summarise OUT/.../NAME_kernel_stats.csv WORKLOAD WIDTH profiles/gcr_multi_flex_trace.json

`run` solves a block of WIDTH right-hand sides once with mgcr_gcr_solve_multi, GCR(5), tol 0, OUTER steps, the LowPrecisionGCR
(GCR(8), 8 steps, tol 0: every inner step of every column runs) in the flexible slot; nothing else touches the device after set-up.
`summarise` adds the entry WORKLOAD/width_WIDTH to the JSON file: kernel time per outer step by family — mflex_* (gate, exit),
g32m_* (the lockstep inner solve), m_* (the batched outer solve's own kernels), everything else (the k-wide fp64 apply, copies).
The solve enqueues OUTER - 1 preconditioned steps, the start's apply and the last step's bookkeeping: the sums are divided by OUTER.
WORKLOAD: lattice, sample or poisson (tools/bench_gcr32_multi.py's)."""
import csv
import json
import os
import re
import sys

import numpy as np

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUTER = 20
STEPS = 8


def run(workload, width):
    from mgpreconditionedgcr_amd import DiracOp, GCR, GCR_Param, LowPrecisionGCR, MultiField, Sparse, _lib, problems
    import bench_gcr32_multi
    for name, n, rp, ci, va, k, _ in bench_gcr32_multi.workloads([workload]):
        M = Sparse(n, n, rp, ci, va)
        A = M if k is None else DiracOp(M, k)
        low = LowPrecisionGCR(M, k, GCR_Param(0, 8, STEPS, 0., False))
        B = MultiField((n,), width, np.array([problems.rhs_grid(n, 8 + j) for j in range(width)], np.complex128))
        X = MultiField((n,), width).set_zero()
        s = GCR(A, GCR_Param(0, 5, OUTER, 0., False, solver_r=low, flexible=True))
        s.solve_multi(B, X)
        _lib.check(_lib.lib().mgcr_synchronize())
        print(name, "rows", n, "width", width, "outer steps", s.last_iterations, "last inner:", low.last_multi())


def summarise(stats_csv, workload, width, out_json):
    fam = {}
    for row in csv.DictReader(open(stats_csv)):
        name = row["Name"]
        m = re.search(r"mgcr::(mflex|g32m|m|q)_(\w+?)_kernel", name)
        family, kernel = (m.group(1), m.group(2)) if m else ("other", re.sub(r"\(.*", "", name.replace("void ", "").replace("mgcr::", ""))[:60])
        e = fam.setdefault(family, {}).setdefault(kernel, dict(calls=0, ns=0))
        e["calls"] += int(row["Calls"])
        e["ns"] += int(row["TotalDurationNs"])
    rec = {"outer_steps": OUTER, "inner_steps_per_apply": STEPS}
    total = 0
    for family, kernels in sorted(fam.items()):
        ns = sum(e["ns"] for e in kernels.values())
        total += ns
        rec[family] = dict(us_per_outer_step=ns / 1e3 / OUTER, launches=sum(e["calls"] for e in kernels.values()),
                           us_per_outer_step_by_kernel={k: e["ns"] / 1e3 / OUTER for k, e in sorted(kernels.items())})
    rec["us_per_outer_step"] = total / 1e3 / OUTER
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    doc["%s/width_%d" % (workload, width)] = rec
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    else:
        summarise(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
