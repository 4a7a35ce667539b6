"""Mixed precision on the even-odd Schur system against the library's other ways to the same solution: wall time per solve of
A x = b to the same true full-system residual 1e-10 |b|, from x = 0, on one MI355X.  Built on tools/bench_gcr32.py.

  (A) mgcr_gcr_solve on the full operator, fp64 GCR(5) alone
  (C) the full operator with LowPrecisionGCR (the fp32 inner solve on the full system) as flexible right preconditioner
  (D) mgcr_eo_solve in fp64, GCR(5) on the Schur system — the best path before this operator, the one to beat
  (E) mgcr_eo_solve with LowPrecisionEvenOddGCR (the fp32 inner solve on the Schur system, csrc/gcr32_eo.hip) in the slot
  (F) mgcr_eo_solve with the library's fp64 nested GCR on the Schur operator in the slot

C, E and F run the same inner settings, (8, 8, 0.1) and (16, 16, 0.01).  Every side is first solved with tolerance 1e-10 and its
tolerance then tightened by the ratio it missed the true residual by (the even-odd solves stop on the Schur residual, every
recurrence residual drifts), so that all stop at the same true residual of the FULL system — formed on the device in fp64 as
|b - A x| / |b| with the full operator.  The timed solves are 6 runs with the sides alternating; medians and ranges.  Workloads: the
3072-row sample at k = 0.18; the periodic 16^4 x 12 lattice with random links at k = 0.116; the same lattice with the twisted
diagonal +- 0.3 i / k; Poisson 128^3 in matrix form.

  python tools/bench_gcr32_eo.py [--only sample,lattice,twisted,poisson] [--runs 6] [--out profiles/gcr32_eo.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import (DiracOp, EvenOddDiagDiracOp, EvenOddSparse, Field, GCR, GCR_Param, LowPrecisionEvenOddGCR,  # noqa: E402
                                     LowPrecisionGCR, Sparse, _lib, problems, stat)
from tests import evenodd_cases as eoc  # noqa: E402
from tests import evenodd_diag_cases as dc  # noqa: E402
from bench_gcr32 import stats  # noqa: E402

TARGET = 1e-10
INNER = ((8, 8, 0.1), (16, 16, 0.01))


def workloads(only):
    if "sample" in only:
        n, rp, ci, va = eoc.load_sample()
        yield "sample_k0.18", n, rp, ci, va, 0.18, 4000
    if "lattice" in only or "twisted" in only:
        n, rp, ci, va = eoc.hopping_lattice((16, 16, 16, 16), 12, True, 14, False)
        if "lattice" in only:
            yield "lattice_16p4x12_k0.116", n, rp, ci, va, 0.116, 4000
        if "twisted" in only:
            d = np.where(np.arange(n) % 2 == 0, 0.3j, -0.3j) / 0.116
            rp2, ci2, va2 = dc.with_diagonal(eoc.Case("lattice", n, rp, ci, va), np.arange(n), d)
            yield "lattice_16p4x12_twisted_k0.116", n, rp2, ci2, va2, 0.116, 4000
    if "poisson" in only:
        n, _, rp, ci, va = problems.poisson3d_csr(128)
        yield "poisson_128", n, rp, ci, va, None, 6000


class Side:
    """one way to the solution: `op` is the system operator, `eo` says which entry point takes it"""

    def __init__(self, name, op, eo, n, cap, precond, full):
        self.name, self.op, self.eo, self.n, self.cap, self.precond, self.full = name, op, eo, n, cap, precond, full
        self.tol = TARGET
        self.times, self.steps, self.res, self.conv = [], 0, 0., False

    def solve(self, b):
        x = Field((self.n,)).set_zero()
        p = GCR_Param(0, 5, self.cap, self.tol, False) if self.precond is None else \
            GCR_Param(0, 5, self.cap, self.tol, False, solver_r=self.precond, flexible=True)
        pc = p._c()
        it, conv = C.c_int32(), C.c_int32()
        fn = _lib.lib().mgcr_eo_solve if self.eo else _lib.lib().mgcr_gcr_solve
        _lib.check(_lib.lib().mgcr_synchronize())
        t0 = time.perf_counter()
        _lib.check(fn(self.op.h, C.byref(pc), b.h, x.h, None, 0, C.byref(it), C.byref(conv)))
        _lib.check(_lib.lib().mgcr_synchronize())
        return time.perf_counter() - t0, it.value, bool(conv.value), x

    def true_residual(self, b, x):
        r = b - self.full(x)
        return float(r.norm() / b.norm())


def overlap(a, b):
    return not (a["min"] > b["max"] or b["min"] > a["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="sample,lattice,twisted,poisson")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcr32_eo.json"))
    args = ap.parse_args()
    out = {"inner_settings": INNER, "target_true_residual": TARGET, "runs": args.runs, "workloads": {}}
    for name, n, rp, ci, va, k, cap in workloads(args.only.split(",")):
        M = Sparse(n, n, rp, ci, va)
        A = M if k is None else DiracOp(M, k)
        S = EvenOddSparse(M) if k is None else EvenOddDiagDiracOp(M, k)
        b = Field((n,), problems.rhs_grid(n, 8))
        rec = {"rows": n, "nnz": int(rp[-1]), "k": k, "sizes": S.sizes()}
        for inner in INNER:
            ip = GCR_Param(0, inner[0], inner[1], inner[2], False)
            low, low_eo, nested = LowPrecisionGCR(M, k, ip), LowPrecisionEvenOddGCR(M, k, ip), GCR(S, ip)
            sides = [Side("A_full_fp64", A, False, n, cap, None, A), Side("C_full_fp32_inner", A, False, n, cap, low, A),
                     Side("D_eo_fp64", S, True, n, cap, None, A), Side("E_eo_fp32_inner", S, True, n, cap, low_eo, A),
                     Side("F_eo_fp64_nested", S, True, n, cap, nested, A)]
            for s in sides:          # calibration (and warm-up): tighten the tolerance until the true residual is at the target
                for _ in range(3):
                    _, it, conv, x = s.solve(b)
                    res = s.true_residual(b, x)
                    if res <= TARGET * 1.001 or not conv:
                        break
                    s.tol *= 0.98 * TARGET / res
                s.res, s.steps, s.conv = res, it, conv
            for _ in range(args.runs):
                for s in sides:
                    before = stat("gcr32_steps")
                    dt, _, _, _ = s.solve(b)
                    s.times.append(dt)
                    s.inner_enqueued = stat("gcr32_steps") - before
            r = {"fp32_eo_info": low_eo.info(), "fp32_full_info": low.info()}
            for s in sides:
                r[s.name] = dict(seconds=stats(s.times), outer_steps=s.steps, converged=s.conv, true_residual=s.res, tol_used=s.tol,
                                 fp32_inner_steps_enqueued=s.inner_enqueued)
            e = r["E_eo_fp32_inner"]["seconds"]
            for other in ("A_full_fp64", "C_full_fp32_inner", "D_eo_fp64", "F_eo_fp64_nested"):
                o = r[other]["seconds"]
                r["E_over_" + other[0]] = o["median"] / e["median"]
                r["ranges_overlap_E_" + other[0]] = overlap(o, e)
            rec["inner_%d_%d_%g" % inner] = r
            print(name, inner, json.dumps(r, default=float), flush=True)
            del low, low_eo, nested, sides
        out["workloads"][name] = rec
        del A, S, M
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, default=float)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
