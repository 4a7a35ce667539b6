"""Kernel time of one LOCKSTEP inner step of the k-wide fp32 inner solve against k single inner steps, for a kernel trace:

  rocprofv3 --kernel-trace --stats -d OUT -o NAME --output-format csv -- python tools/trace_gcr32_multi.py run WORKLOAD WIDTH
  python tools/trace_gcr32_multi.py summarise OUT/.../NAME_kernel_stats.csv WORKLOAD WIDTH profiles/gcr32_multi_trace.json

`run` applies the batched inner solve (LowPrecisionGCR.inner_multi) REPS times to a block of WIDTH right-hand sides and the single
inner solve REPS times to each of its columns — GCR(8), 8 steps, tol 0, so every step of every column runs; nothing else touches the
device after set-up.  In the trace the g32m_* kernels are the batched side's and the g32_* kernels the single side's.
`summarise` adds the entry WORKLOAD/width_WIDTH to the JSON file: kernel time per lockstep step (all g32m_* kernels / (REPS x 8)),
per k single steps (all g32_* kernels / (REPS x 8), which already covers the WIDTH columns), and the per-kernel-family split of
both.  WORKLOAD: lattice, sample or poisson (tools/bench_gcr32_multi.py's)."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS = 5
STEPS = 8


def run(workload, width):
    from mgpreconditionedgcr_amd import Field, GCR_Param, LowPrecisionGCR, MultiField, Sparse, _lib, problems
    import bench_gcr32_multi
    for name, n, rp, ci, va, k, _ in bench_gcr32_multi.workloads([workload]):
        M = Sparse(n, n, rp, ci, va)
        low = LowPrecisionGCR(M, k, GCR_Param(0, 8, STEPS, 0., False))
        fs = [Field((n,), problems.rhs_grid(n, 8 + j)) for j in range(width)]
        F, Y, y = MultiField.from_fields(fs), MultiField((n,), width), Field((n,))
        for _ in range(REPS):
            low.inner_multi(F, Y)
        _lib.check(_lib.lib().mgcr_synchronize())
        for _ in range(REPS):
            for f in fs:
                low(f, y)
        _lib.check(_lib.lib().mgcr_synchronize())
        print(name, "rows", n, "width", width, "reps", REPS, "inner steps per apply", STEPS, "batched last:", low.last_multi())


def summarise(stats_csv, workload, width, out_json):
    fam = {"multi": {}, "single": {}}
    for row in csv.DictReader(open(stats_csv)):
        m = re.search(r"mgcr::(g32m?)_(\w+?)_kernel", row["Name"])
        if not m:
            continue
        side = fam["multi" if m.group(1) == "g32m" else "single"]
        e = side.setdefault(m.group(2), dict(calls=0, ns=0))
        e["calls"] += int(row["Calls"])
        e["ns"] += int(row["TotalDurationNs"])
    rec = {}
    for side, kernels in fam.items():
        total = sum(e["ns"] for e in kernels.values())
        rec[side] = dict(us_per_step=total / 1e3 / (REPS * STEPS), launches=sum(e["calls"] for e in kernels.values()),
                         us_per_step_by_kernel={k: e["ns"] / 1e3 / (REPS * STEPS) for k, e in sorted(kernels.items())})
    rec["k_single_steps_over_one_lockstep_step"] = rec["single"]["us_per_step"] / rec["multi"]["us_per_step"]
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {
        "what": "rocprofv3 --kernel-trace --stats of tools/trace_gcr32_multi.py: kernel time of one lockstep inner step at width k "
                "(multi) against k single inner steps (single), entry and exit launches included", "reps": REPS, "inner_steps_per_apply": STEPS,
        "workloads": {}}
    doc["workloads"]["%s/width_%d" % (workload, width)] = rec
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    else:
        summarise(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
