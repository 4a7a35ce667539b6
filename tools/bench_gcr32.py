"""Mixed precision against fp64: wall time per solve of A x = b to the same true residual 1e-10 |b|, from x = 0, on one MI355X.

  (A) mgcr_gcr_solve, fp64 GCR(5) alone
  (B) fp64 flexible GCR(5), right preconditioner = the library's fp64 nested GCR (mgcr_gcr_create(A, inner, x0_mode = 1))
  (C) fp64 flexible GCR(5), right preconditioner = LowPrecisionGCR (the fp32 inner solve, csrc/gcr32.hip)

B and C run the same inner settings (--inner restart,max_iter,tol).  Every side is first solved once with tolerance 1e-10 and its
tolerance then tightened by the ratio it missed the true residual 1e-10 by (the recurrence residual drifts), so that all three stop at
the same true residual; the timed solves are 6 runs with the sides alternating A, B, C, A, B, C, ...; medians and ranges are
reported (a wall-time quotient per inner step is stored too, outer share included: tools/trace_gcr32.py has the kernel times).  Workloads: the 3072-row sample at
k = 0.18, Poisson 128^3 in matrix form, the scattered irregular CSR of 2^20 rows (problems.skewed_csr, window 2^17) in Dirac form,
the periodic 16^4 x 12 lattice with random links at k = 0.116.

  python tools/bench_gcr32.py [--only sample,poisson,irregular,lattice] [--runs 6] [--out profiles/gcr32.json]
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
from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, LowPrecisionGCR, Sparse, _lib, problems, stat  # noqa: E402
from tests import evenodd_cases as eoc  # noqa: E402

TARGET = 1e-10


def workloads(only):
    if "sample" in only:
        n, rp, ci, va = eoc.load_sample()
        yield "sample_k0.18", n, rp, ci, va, 0.18, 4000
    if "poisson" in only:
        n, _, rp, ci, va = problems.poisson3d_csr(128)
        yield "poisson_128", n, rp, ci, va, None, 6000
    if "irregular" in only:
        n = 1 << 20
        rp, ci, va = problems.skewed_csr(n, np.random.default_rng(4), window=1 << 17)
        lens = np.diff(rp)
        k = 0.5 / (np.sqrt(lens.mean()) * np.sqrt(np.mean(np.abs(va) ** 2)))
        yield "skewed_2p20", n, rp, ci, va, float(k), 2000
    if "lattice" in only:
        n, rp, ci, va = eoc.hopping_lattice((16, 16, 16, 16), 12, True, 14, False)
        yield "lattice_16p4x12_k0.116", n, rp, ci, va, 0.116, 4000


def true_residual(n, rp, ci, va, k, b, x):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    s = np.zeros(n, np.complex128)
    s.real = np.bincount(rows, (va * x[ci]).real, n)
    s.imag = np.bincount(rows, (va * x[ci]).imag, n)
    ax = s if k is None else x - k * s
    return float(np.linalg.norm(b - ax) / np.linalg.norm(b))


class Side:
    def __init__(self, name, A, n, cap, precond):
        self.name, self.A, self.n, self.cap, self.precond = name, A, n, cap, precond
        self.tol = TARGET
        self.times, self.steps, self.res = [], 0, 0.

    def param(self):
        if self.precond is None:
            return GCR_Param(0, 5, self.cap, self.tol, False)
        return GCR_Param(0, 5, self.cap, self.tol, False, solver_r=self.precond, flexible=True)

    def solve(self, b):
        x = Field((self.n,)).set_zero()
        pc = self.param()._c()
        it, conv = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().mgcr_synchronize())
        t0 = time.perf_counter()
        _lib.check(_lib.lib().mgcr_gcr_solve(self.A.h, C.byref(pc), b.h, x.h, None, 0, C.byref(it), C.byref(conv)))
        _lib.check(_lib.lib().mgcr_synchronize())
        dt = time.perf_counter() - t0
        return dt, it.value, bool(conv.value), x


def stats(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="sample,poisson,irregular,lattice")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--inner", default="8,8,0.1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcr32.json"))
    args = ap.parse_args()
    r, m, t = args.inner.split(",")
    inner = (int(r), int(m), float(t))
    out = {"inner": inner, "target_true_residual": TARGET, "runs": args.runs, "workloads": {}}
    for name, n, rp, ci, va, k, cap in workloads(args.only.split(",")):
        M = Sparse(n, n, rp, ci, va)
        A = M if k is None else DiracOp(M, k)
        bh = problems.rhs_grid(n, 8)
        b = Field((n,), bh)
        ip = GCR_Param(0, inner[0], inner[1], inner[2], False)
        nested = GCR(A, ip)
        low = LowPrecisionGCR(M, k, ip)
        sides = [Side("A_fp64", A, n, cap, None), Side("B_fp64_nested", A, n, cap, nested), Side("C_fp32_inner", A, n, cap, low)]
        rec = {"rows": n, "nnz": int(rp[-1]), "k": k, "fp32_info": low.info(), "fp64_stored": M.stored_bytes()}
        for s in sides:          # calibration (and warm-up): tighten the tolerance until the true residual is at the target
            for _ in range(3):
                _, it, conv, x = s.solve(b)
                res = true_residual(n, rp, ci, va, k, bh, x.to_numpy())
                if res <= TARGET * 1.001 or not conv:
                    break
                s.tol *= 0.98 * TARGET / res
            s.res, s.steps, s.conv = res, it, conv
        for _ in range(args.runs):
            for s in sides:
                before = stat("gcr32_steps")
                dt, it, conv, _ = s.solve(b)
                s.times.append(dt)
                s.inner_enqueued = stat("gcr32_steps") - before if s.precond is low else (it + 1) * inner[1] if s.precond else 0
        for s in sides:
            st = stats(s.times)
            rec[s.name] = dict(seconds=st, outer_steps=s.steps, converged=s.conv, true_residual=s.res, tol_used=s.tol,
                               inner_steps_enqueued=s.inner_enqueued,
                               us_per_inner_step=1e6 * st["median"] / s.inner_enqueued if s.inner_enqueued else None,
                               us_per_outer_step=1e6 * st["median"] / max(s.steps, 1))
        a, bb, c = (rec[s.name]["seconds"] for s in sides)
        rec["C_over_A"] = a["median"] / c["median"]
        rec["C_over_B"] = bb["median"] / c["median"]
        rec["ranges_overlap_A_C"] = not (a["min"] > c["max"] or c["min"] > a["max"])
        rec["ranges_overlap_B_C"] = not (bb["min"] > c["max"] or c["min"] > bb["max"])
        out["workloads"][name] = rec
        print(name, json.dumps(rec, default=float), flush=True)
        del nested, low, sides, A, M
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, default=float)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
