"""The flexible batched GCR against the other ways to solve A X = B for a block of k right-hand sides to the same true residual
1e-10 |b_j| per column, from X = 0, on one MI355X: wall time per BLOCK.  Same method as tools/bench_gcr32_multi.py (whose sides A, B
and E this tool runs unchanged), same workloads, same inner settings.

  (A) k x mgcr_gcr_solve, fp64 flexible GCR(5) with LowPrecisionGCR in the right_precond slot
  (B) mgcr_gcr_solve_multi, the batched fp64 GCR(5) at width k, unpreconditioned
  (E) mgcr_gcr32_solve_multi, fp64 defect correction around the k-wide lockstep inner solve
  (F) mgcr_gcr_solve_multi with the LowPrecisionGCR in the right_precond slot, flexible = 1: the batched GCR(5) around the k-wide
      lockstep inner solve (csrc/gcr_multi.hip, csrc/gcr_multi_flex.hip) — column j has the bits of (A)'s solve of column j

Every side is first solved once with tolerance 1e-10 and its tolerance then tightened by the ratio its worst column missed the true
residual by, so all stop at the same true residual (measured on the device with the fp64 operator); a side that does not reach it
within its step cap is recorded as not converged, with the residual it reached.  The timed solves are `--runs` runs with the sides
alternating A, B, E, F, A, ...; medians and ranges are reported.  --time-limit S: a configuration is started only while fewer than S
seconds have passed; the ones left out are listed as not measured.

  python tools/bench_gcr_multi_flex.py [--only lattice,sample,poisson] [--widths 4,8,12] [--inner 8,8,0.1 --inner 8,32,1e-3] [--runs 6]
                                       [--time-limit 1000] [--out profiles/gcr_multi_flex.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import DiracOp, GCR_Param, LowPrecisionGCR, MultiField, Sparse, _lib, problems, stat  # noqa: E402
from bench_gcr32_multi import TARGET, Bench, stats, sync, workloads  # noqa: E402


class FlexBench(Bench):
    def side_f(self, tol):
        pc = GCR_Param(0, 5, self.cap, tol, False, solver_r=self.low, flexible=True)._c()
        X = MultiField((self.n,), self.k).set_zero()
        it = (C.c_int32 * self.k)()
        sync()
        t0 = time.perf_counter()
        _lib.check(_lib.lib().mgcr_gcr_solve_multi(self.A.h, C.byref(pc), self.B.h, X.h, None, 0, it, None))
        sync()
        dt = time.perf_counter() - t0
        return dt, [X.column(j) for j in range(self.k)], list(it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="lattice,sample,poisson")
    ap.add_argument("--widths", default="4,8,12")
    ap.add_argument("--inner", action="append")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--time-limit", type=float, default=1e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcr_multi_flex.json"))
    args = ap.parse_args()
    inners = [(int(r), int(m), float(t)) for r, m, t in (s.split(",") for s in (args.inner or ["8,8,0.1", "8,32,1e-3"]))]
    widths = [int(w) for w in args.widths.split(",")]
    out = {"target_true_residual": TARGET, "runs": args.runs, "workloads": {}, "not_measured": []}
    if os.path.exists(args.out):          # (a run per workload adds to the file)
        old = json.load(open(args.out))
        if old.get("target_true_residual") == TARGET and old.get("runs") == args.runs:
            out["workloads"].update(old.get("workloads", {}))
            out["not_measured"] = [k for k in old.get("not_measured", [])]
    start = time.perf_counter()

    def save():
        out["not_measured"] = sorted(set(out["not_measured"]) - set(out["workloads"]))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True, default=float)

    for name, n, rp, ci, va, kk, cap in workloads(args.only.split(",")):
        M = Sparse(n, n, rp, ci, va)
        A = M if kk is None else DiracOp(M, kk)
        for inner in inners:
            low = LowPrecisionGCR(M, kk, GCR_Param(0, inner[0], inner[1], inner[2], False))
            for k in widths:
                key = "%s/inner_%d_%d_%g/width_%d" % (name, inner[0], inner[1], inner[2], k)
                if time.perf_counter() - start > args.time_limit:
                    out["not_measured"].append(key)
                    print(key, "NOT measured: the time limit was reached", flush=True)
                    save()
                    continue
                bench = FlexBench(A, low, n, k, cap, [problems.rhs_grid(n, 8 + j) for j in range(k)])
                sides = {"A_k_single_mixed": bench.side_a, "B_fp64_batched": bench.side_b, "E_batched_defect": bench.side_e,
                         "F_batched_flexible": bench.side_f}
                tol, rec = {}, {"rows": n, "nnz": int(rp[-1]), "k": kk, "width": k, "inner": inner}
                for s, fn in sides.items():          # calibration (and warm-up): tighten the tolerance until the worst column is at the target
                    tol[s] = TARGET
                    for _ in range(3):
                        before = stat("gcr32_multi_applies")
                        _, xs, steps = fn(tol[s])
                        res = bench.worst(xs)
                        applies = stat("gcr32_multi_applies") - before
                        if res <= TARGET * 1.001 or s == "E_batched_defect":          # (E tests the true residual itself: a miss is the step cap)
                            break
                        tol[s] *= 0.98 * TARGET / res
                    rec[s] = dict(true_residual_worst=res, converged=bool(res <= TARGET * 1.001), steps=steps, tol_used=tol[s],
                                  batched_applies_enqueued=applies)
                times = {s: [] for s in sides}
                for _ in range(args.runs):
                    for s, fn in sides.items():
                        times[s].append(fn(tol[s])[0])
                for s in sides:
                    rec[s]["seconds_per_block"] = stats(times[s])
                f = rec["F_batched_flexible"]["seconds_per_block"]
                for s in ("A_k_single_mixed", "B_fp64_batched", "E_batched_defect"):
                    o = rec[s]["seconds_per_block"]
                    rec["F_speedup_over_" + s[0]] = o["median"] / f["median"]
                    rec["ranges_overlap_F_" + s[0]] = not (o["min"] > f["max"] or f["min"] > o["max"])
                out["workloads"][key] = rec
                print(key, json.dumps(rec, default=float), flush=True)
                save()          # (after every entry: a run that is cut short keeps what it measured)
                del bench
            del low
        del A, M
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
