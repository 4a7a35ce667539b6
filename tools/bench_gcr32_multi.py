"""Batched mixed precision against the other ways to solve A X = B for a block of k right-hand sides to the same true residual
1e-10 |b_j| per column, from X = 0, on one MI355X: wall time per BLOCK.

  (A) k x mgcr_gcr_solve, fp64 flexible GCR(5) with LowPrecisionGCR in the right_precond slot — the best single mixed path
  (B) mgcr_gcr_solve_multi, the batched fp64 GCR(5) at width k, unpreconditioned
  (C) k x the single-column defect-correction loop (mgcr_op_apply, mgcr_add_scaled, mgcr_norm2, mgcr_axpy around the single inner
      solve): what (E) computes, one column at a time — it isolates what batching buys
  (E) mgcr_gcr32_solve_multi, fp64 defect correction around the k-wide lockstep inner solve (csrc/gcr32_multi.hip)

A, C and E run the same inner settings.  Every side is first solved once with tolerance 1e-10 and its tolerance then tightened by the
ratio its worst column missed the true residual 1e-10 by (the recurrence residual of A and B drifts; C and E test the true residual
itself), so all four stop at the same true residual (measured on the device with the fp64 operator); the timed solves are `--runs`
runs with the sides alternating A, B, C, E, A, ...; medians and ranges are reported.  Workloads: the periodic 16^4 x 12 lattice with
random links at k = 0.116, the 3072-row sample at k = 0.18, Poisson 128^3 in matrix form.

  python tools/bench_gcr32_multi.py [--only lattice,sample,poisson] [--widths 4,8,12] [--inner 8,8,0.1 --inner 8,32,1e-3] [--runs 6]
                                    [--out profiles/gcr32_multi.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mgpreconditionedgcr_amd import DiracOp, Field, GCR_Param, LowPrecisionGCR, MultiField, Sparse, _lib, problems  # noqa: E402
from tests import evenodd_cases as eoc  # noqa: E402

TARGET = 1e-10
MAX_OUTER = 400


def workloads(only):
    if "lattice" in only:
        n, rp, ci, va = eoc.hopping_lattice((16, 16, 16, 16), 12, True, 14, False)
        yield "lattice_16p4x12_k0.116", n, rp, ci, va, 0.116, 4000
    if "sample" in only:
        n, rp, ci, va = eoc.load_sample()
        yield "sample_k0.18", n, rp, ci, va, 0.18, 4000
    if "poisson" in only:
        n, _, rp, ci, va = problems.poisson3d_csr(128)
        yield "poisson_128", n, rp, ci, va, None, 6000


def sync():
    _lib.check(_lib.lib().mgcr_synchronize())


class Bench:
    def __init__(self, A, low, n, k, cap, bs):
        self.A, self.low, self.n, self.k, self.cap = A, low, n, k, cap
        self.b = [Field((n,), v) for v in bs]
        self.B = MultiField.from_fields(self.b)
        self.bnorm = [f.norm() for f in self.b]

    def worst(self, xs):
        """the worst column's true residual, with the fp64 operator on the device"""
        return max((b.add_scaled(-1.0, self.A(x))).norm() / bn for b, x, bn in zip(self.b, xs, self.bnorm))

    def side_a(self, tol):
        pc = GCR_Param(0, 5, self.cap, tol, False, solver_r=self.low, flexible=True)._c()
        xs, steps = [Field((self.n,)).set_zero() for _ in range(self.k)], []
        sync()
        t0 = time.perf_counter()
        for b, x in zip(self.b, xs):
            it, conv = C.c_int32(), C.c_int32()
            _lib.check(_lib.lib().mgcr_gcr_solve(self.A.h, C.byref(pc), b.h, x.h, None, 0, C.byref(it), C.byref(conv)))
            steps.append(it.value)
        sync()
        return time.perf_counter() - t0, xs, steps

    def side_b(self, tol):
        pc = GCR_Param(0, 5, self.cap, tol, False)._c()
        X = MultiField((self.n,), self.k).set_zero()
        it = (C.c_int32 * self.k)()
        sync()
        t0 = time.perf_counter()
        _lib.check(_lib.lib().mgcr_gcr_solve_multi(self.A.h, C.byref(pc), self.B.h, X.h, None, 0, it, None))
        sync()
        dt = time.perf_counter() - t0
        return dt, [X.column(j) for j in range(self.k)], list(it)

    def side_c(self, tol):
        xs, steps = [], []
        sync()
        t0 = time.perf_counter()
        for b in self.b:
            x = Field((self.n,)).set_zero()
            r = b.copy()
            b2, r2, t = b.squarednorm(), None, 0
            r2 = r.squarednorm()
            while r2 > tol * tol * b2 and t < MAX_OUTER:
                t += 1
                x += self.low(r)
                r = b.add_scaled(-1.0, self.A(x))
                r2 = r.squarednorm()
            xs.append(x)
            steps.append(t)
        sync()
        return time.perf_counter() - t0, xs, steps

    def side_e(self, tol):
        X = MultiField((self.n,), self.k).set_zero()
        sync()
        t0 = time.perf_counter()
        self.low.solve_multi(self.A, self.B, X, tol=tol, max_outer=MAX_OUTER)
        sync()
        dt = time.perf_counter() - t0
        return dt, [X.column(j) for j in range(self.k)], list(self.low.last_iterations)


def stats(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="lattice,sample,poisson")
    ap.add_argument("--widths", default="4,8,12")
    ap.add_argument("--inner", action="append")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcr32_multi.json"))
    args = ap.parse_args()
    inners = [(int(r), int(m), float(t)) for r, m, t in (s.split(",") for s in (args.inner or ["8,8,0.1", "8,32,1e-3"]))]
    widths = [int(w) for w in args.widths.split(",")]
    out = {"target_true_residual": TARGET, "runs": args.runs, "workloads": {}}
    for name, n, rp, ci, va, kk, cap in workloads(args.only.split(",")):
        M = Sparse(n, n, rp, ci, va)
        A = M if kk is None else DiracOp(M, kk)
        for inner in inners:
            low = LowPrecisionGCR(M, kk, GCR_Param(0, inner[0], inner[1], inner[2], False))
            for k in widths:
                bench = Bench(A, low, n, k, cap, [problems.rhs_grid(n, 8 + j) for j in range(k)])
                sides = {"A_k_single_mixed": bench.side_a, "B_fp64_batched": bench.side_b, "C_k_single_defect": bench.side_c,
                         "E_batched_mixed": bench.side_e}
                tol, rec = {}, {"rows": n, "nnz": int(rp[-1]), "k": kk, "width": k, "inner": inner}
                for s, fn in sides.items():          # calibration (and warm-up): tighten the tolerance until the worst column is at the target
                    tol[s] = TARGET
                    for _ in range(3):
                        _, xs, steps = fn(tol[s])
                        res = bench.worst(xs)
                        if res <= TARGET * 1.001:
                            break
                        tol[s] *= 0.98 * TARGET / res
                    rec[s] = dict(true_residual_worst=res, steps=steps, tol_used=tol[s])
                times = {s: [] for s in sides}
                for _ in range(args.runs):
                    for s, fn in sides.items():
                        times[s].append(fn(tol[s])[0])
                for s in sides:
                    rec[s]["seconds_per_block"] = stats(times[s])
                e = rec["E_batched_mixed"]["seconds_per_block"]
                for s in ("A_k_single_mixed", "B_fp64_batched", "C_k_single_defect"):
                    o = rec[s]["seconds_per_block"]
                    rec["E_speedup_over_" + s[0]] = o["median"] / e["median"]
                    rec["ranges_overlap_E_" + s[0]] = not (o["min"] > e["max"] or e["min"] > o["max"])
                key = "%s/inner_%d_%d_%g/width_%d" % (name, inner[0], inner[1], inner[2], k)
                out["workloads"][key] = rec
                print(key, json.dumps(rec, default=float), flush=True)
                with open(args.out, "w") as f:          # (after every entry: a run that is cut short keeps what it measured)
                    json.dump(out, f, indent=1, sort_keys=True, default=float)
                del bench
            del low
        del A, M
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, default=float)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
