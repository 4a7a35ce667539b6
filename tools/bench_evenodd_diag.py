#!/usr/bin/env python3
"""Even-odd Schur solve of an operator WITH a site diagonal (mgcr_eo_create_diag) against the full solve, stopped at the same true
residual: GCR(5) from x0 = 0 down to 1e-8 |b| on both sides.

  side A  mgcr_gcr_solve on the full operator (the Sparse itself, or DiracOp(D, k) with D holding the diagonal), tol 1e-8;
  side B  mgcr_eo_solve (EvenOddSparse / EvenOddDiagDiracOp .solve: prepare, GCR on the Schur system of the even half, reconstruct)
          with tol 1e-8 |b| / |bhat_e| — the Schur history is relative to |bhat_e| and the full system's true residual is
          hist[last] |bhat_e| / |b| (include/mgcr.h).

Problems: the 7-point Poisson matrix of an n^3 box in matrix form (--poisson 128 256), and the periodic 16^4 x 12 lattice of
tools/bench_evenodd.py with a twisted diagonal d = +- 0.3 i / k (Dirac form, k = --k-synth).  The sides ALTERNATE in one process,
--runs (>= 6) timings each after one untimed pass; medians and ranges, `ranges_overlap` says where no claim can be made.  Per side:
steps, wall time per solve (host clock around the call, device idle before and after), wall time / steps — which carries the
per-solve part — and the true residual |A x - b| / |b| of the LAST solve, computed on the device through the full operator.
Also the Schur apply alone (mgcr_bench_op_apply, device events, 20 applies) against its byte model (site diagonal):
both halves' stored bytes once, x gathered and t gathered once each (counted as one pass over a half vector), 1/a_o, a_e and w
streamed, t and y written: M + 4 V_e + 3 V_o with V = 16 B per entry.
One JSON line to stdout; --out FILE (default profiles/evenodd_diag.json) writes it too.  No torch import."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import DiracOp, EvenOddDiagDiracOp, EvenOddSparse, Field, GCR_Param, Sparse, _lib, problems  # noqa: E402
from bench_evenodd import overlap, solve_call, stats, synthetic, wall_ms  # noqa: E402

RESTART, TOL = 5, 1e-8


def twisted_lattice(k):
    """The hopping matrix of tools/bench_evenodd.py with one diagonal entry per row, d = +- 0.3 i / k alternating from row to row
    (stored first in its row)"""
    n, rowptr, col, val = synthetic()
    per = int(rowptr[1])
    col2 = np.empty((n, per + 1), np.int64)
    val2 = np.empty((n, per + 1), np.complex128)
    col2[:, 0] = np.arange(n)
    val2[:, 0] = np.where(np.arange(n) % 2 == 0, 0.3j, -0.3j) / k
    col2[:, 1:] = col.reshape(n, per)
    val2[:, 1:] = val.reshape(n, per)
    return n, np.arange(n + 1, dtype=np.int64) * (per + 1), col2.reshape(-1), val2.reshape(-1)


def true_residual(full, b, x, n):
    r = full(x)
    return float(np.sqrt(b.add_scaled(-1.0, r).squarednorm() / b.squarednorm()))


def compare(name, full, eo, n, runs, cap):
    b = Field((n,)).fill_rhs(1)
    x = Field((n,))
    bnorm = float(np.sqrt(b.squarednorm()))
    bhat_norm = float(np.sqrt(eo.prepare(b).squarednorm()))
    prm_a = GCR_Param(0, RESTART, cap, TOL, False, check_every=50)
    prm_b = GCR_Param(0, RESTART, cap, TOL * bnorm / bhat_norm, False, check_every=50)
    a = solve_call(full, prm_a, b, x.set_zero(), cap + 1)             # untimed pass of each side
    eo.solve(b, x.set_zero(), prm_b)
    print("%s: full %d steps, even-odd %d steps" % (name, a[0], eo.last_iterations), file=sys.stderr, flush=True)
    t_a, t_b = [], []
    for _ in range(runs):
        x.set_zero()
        t_a.append(wall_ms(lambda: solve_call(full, prm_a, b, x, cap + 1)))
        res_a = true_residual(full, b, x, n)
        x.set_zero()
        t_b.append(wall_ms(lambda: eo.solve(b, x, prm_b)))
        res_b = true_residual(full, b, x, n)
        print("%s: full %.1f ms, even-odd %.1f ms" % (name, t_a[-1], t_b[-1]), file=sys.stderr, flush=True)
    sa, sb = stats(t_a), stats(t_b)
    h_eo, h_oe = eo.halves()
    ne, no = eo.sizes()[1:]
    xe, ye = Field((ne,)).fill_rhs(2), Field((ne,))
    apply_ms = eo.bench_apply(xe, ye, 20)
    model = h_eo.stored_bytes()["matrix_bytes"] + h_oe.stored_bytes()["matrix_bytes"] + 16.0 * (4 * ne + 3 * no)
    return {"problem": name, "rows": n, "n_even": ne, "n_odd": no, "tol_true_residual": TOL, "schur_tol": TOL * bnorm / bhat_norm,
            "full": {"ms": sa, "steps": a[0], "converged": a[1], "us_per_step": 1e3 * sa["median"] / max(a[0], 1), "true_residual": res_a},
            "evenodd": {"ms": sb, "steps": eo.last_iterations, "converged": eo.last_converged,
                        "us_per_step": 1e3 * sb["median"] / max(eo.last_iterations, 1), "true_residual": res_b},
            "wall_ratio_full_over_evenodd": sa["median"] / sb["median"], "ranges_overlap": overlap(sa, sb),
            "schur_apply": {"us": 1e3 * apply_ms, "byte_model": model, "model_gb_per_s": model / (1e6 * apply_ms)},
            "half_storage": {"H_eo": {"format": h_eo.storage_format()[0], **h_eo.ell_layout()},
                             "H_oe": {"format": h_oe.storage_format()[0], **h_oe.ell_layout()}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poisson", type=int, nargs="*", default=[128, 256], help="box sizes n of the n^3 Poisson problems")
    ap.add_argument("--lattice", type=int, default=1, help="0: skip the twisted 16^4 x 12 lattice")
    ap.add_argument("--k-synth", type=float, default=0.116)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--cap", type=int, default=200000, help="step cap of every solve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evenodd_diag.json"))
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import bench
    _lib.init()
    out = {"src_sha16": bench.source_sha16(), "restart": RESTART, "runs": a.runs, "step_cap": a.cap, "cases": []}
    for n in a.poisson:
        N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
        A = Sparse(N, ncol, rowptr, col, val)
        out["cases"].append(compare("poisson_%d^3" % n, A, EvenOddSparse(A), N, a.runs, a.cap))
        del A
    if a.lattice:
        n, rowptr, col, val = twisted_lattice(a.k_synth)
        D = Sparse(n, n, rowptr, col, val)
        case = compare("twisted_16x16x16x16x12", DiracOp(D, a.k_synth), EvenOddDiagDiracOp(D, a.k_synth), n, a.runs, a.cap)
        case["k"] = a.k_synth
        out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
