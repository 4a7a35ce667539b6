#!/usr/bin/env python3
"""Even-odd hopping-parameter scans: one batched Schur solve (MultiEvenOddDiracOp.solve, mgcr_eo_multi_solve) against the two forms a
scan had before it.  Same right-hand side in every column, GCR(5), tol 1e-10.

One JSON line to stdout; --out FILE (default profiles/evenodd_multi.json) writes it too, stamped with the fingerprint of the kernel
sources (bench.source_sha16).  Sides, ALTERNATING in one process, --runs (>= 6) timings each after one untimed pass, medians and
ranges (`ranges_overlap_*` says where no claim can be made):
  A  evenodd_ladder   mgcr_eo_solve per value, mgcr_eo_set_k between them, the operator's solver state kept: fewer steps, one k at a time;
  B  full_batched     mgcr_gcr_solve_multi on MultiDiracOp(D, ks): shared steps, the FULL system;
  C  evenodd_batched  mgcr_eo_multi_solve: both.
Problems:
  (a) the 3072-row sample (--sample FILE, text CSR), the ladder 0.05, 0.10, 0.15, 0.15+0.05i, 0.18, 0.20, step cap 200, wall time;
  (b) the periodic 16^4 x 12 lattice of tools/bench_evenodd.py (786 432 rows), 4 and 8 values around 0.116, step cap 4000.
A batched solve runs as long as its slowest column: `sum_over_max` = sum of the columns' iteration counts / the largest — the number
of system-iterations a lockstep step is worth on average; C beats A where that exceeds C's step cost / A's step cost.
`step_cost`: tol 0 at two step caps N1 < N2 on convergent values, per-step cost = (t(N2) - t(N1)) / (N2 - N1) and the same per
system-iteration (/ k for the batched sides).  Byte model next to it (M = 20 B per stored entry of D, V = 16 n): the Schur step
streams both halves of D once for the whole block and k columns of the single Schur step's vector traffic, M + k 8.8 V.
No torch import."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import (EvenOddDiracOp, Field, GCR, GCR_Param, MultiDiracOp, MultiEvenOddDiracOp, MultiField, Sparse, _lib,  # noqa: E402
                                     read_data)
from bench_evenodd import overlap, stats, synthetic, wall_ms  # noqa: E402

RESTART, TOL = 5, 1e-10
SAMPLE_LADDER = [0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18, 0.20]


def sides(D, eo, n, ks, cap, tol):
    """the three ways to run the ladder; each returns the columns' iteration counts"""
    k = len(ks)
    prm = GCR_Param(0, RESTART, cap, tol, False, check_every=50)
    b = Field((n,)).fill_rhs(1)
    B = MultiField.from_fields([b] * k)
    scan = MultiEvenOddDiracOp(eo, ks)        # (eo: ONE EvenOddDiracOp per matrix — side A walks it with set_k, side C borrows its halves)
    full = GCR(MultiDiracOp(D, ks), prm)
    x, X = Field((n,)), MultiField((n,), k)

    def ladder():
        its = []
        for kj in ks:
            eo.set_k(kj)
            eo.solve(b, x.set_zero(), prm)
            its.append(eo.last_iterations)
        return its

    def full_batched():
        full.solve_multi(B, X.set_zero())
        return list(full.last_iterations)

    def evenodd_batched():
        scan.solve(B, X.set_zero(), prm)
        return list(scan.last_iterations)

    return {"evenodd_ladder": ladder, "full_batched": full_batched, "evenodd_batched": evenodd_batched}


def timed(fns, runs):
    its, t = {}, {name: [] for name in fns}
    for r in range(runs + 1):
        for name, fn in fns.items():
            box = {}
            ms = wall_ms(lambda: box.update(its=fn()))
            its[name] = box["its"]
            if r:
                t[name].append(ms)
    return its, {name: stats(v) for name, v in t.items()}


def compare(D, eo, n, ks, cap, runs):
    its, ms = timed(sides(D, eo, n, ks, cap, TOL), runs)
    out = {"ks": [[complex(z).real, complex(z).imag] for z in ks], "step_cap": cap}
    for name in ms:
        out[name] = {"ms": ms[name], "iterations": its[name], "sum_over_max": sum(its[name]) / max(max(its[name]), 1)}
    c = ms["evenodd_batched"]
    for name, key in (("evenodd_ladder", "A"), ("full_batched", "B")):
        out["wall_ratio_%s_over_C" % key] = ms[name]["median"] / c["median"]
        out["ranges_overlap_%s" % key] = overlap(ms[name], c)
    return out


def step_cost(D, eo, n, ks, runs, n1, n2):
    k = len(ks)
    fns = {m: sides(D, eo, n, ks, m, 0.0) for m in (n1, n2)}
    t = {(name, m): [] for name in fns[n1] for m in (n1, n2)}
    for r in range(runs + 1):
        for m in (n1, n2):
            for name, fn in fns[m].items():
                box = {}
                ms = wall_ms(lambda: box.update(its=fn()))
                assert box["its"] == [m] * k, (name, m, box["its"])
                if r:
                    t[(name, m)].append(ms)
    M, V = 20.0 * D.get_nnz(), 16.0 * n
    out = {"ks": [[complex(z).real, complex(z).imag] for z in ks], "steps": [n1, n2],
           "byte_model": {"M": M, "V": V, "evenodd_batched_bytes_per_step": M + k * 8.8 * V, "evenodd_single_bytes_per_step": M + 8.8 * V}}
    for name in fns[n1]:
        a, c = stats(t[(name, n1)]), stats(t[(name, n2)])
        # the ladder runs k solves of N steps each: its "step" below is one step of ONE system
        systems_per_step = 1 if name == "evenodd_ladder" else k
        per = (c["median"] - a["median"]) / (n2 - n1) / (k if name == "evenodd_ladder" else 1)
        out[name] = {"ms_at_n1": a, "ms_at_n2": c, "us_per_step": 1e3 * per, "us_per_system_iteration": 1e3 * per / systems_per_step}
    out["evenodd_batched"]["model_TB_per_s"] = out["byte_model"]["evenodd_batched_bytes_per_step"] / (out["evenodd_batched"]["us_per_step"] * 1e-6) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", default=None, help="the 3072-row sample matrix (text CSR, e.g. 4x4parsed.txt); omitted: problem (a) is skipped")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--k-synth", type=float, default=0.116)
    ap.add_argument("--parts", nargs="+", default=["sample", "synthetic"], choices=["sample", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evenodd_multi.json"))
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import bench
    _lib.init()
    out = {"src_sha16": bench.source_sha16(), "restart": RESTART, "tol": TOL, "runs": a.runs, "problems": {}}
    if "sample" in a.parts and a.sample:
        D = read_data(os.path.basename(a.sample), directory=os.path.dirname(os.path.abspath(a.sample)))
        n = D.get_dim()
        eo = EvenOddDiracOp(D, SAMPLE_LADDER[0])
        out["problems"]["sample"] = {"rows": n, "nnz": D.get_nnz(), "ladder": compare(D, eo, n, SAMPLE_LADDER, 200, a.runs),
                                     "step_cost": step_cost(D, eo, n, [0.13 + 0.004 * j for j in range(6)], a.runs, 50, 250)}
    if "synthetic" in a.parts:
        n, rowptr, col, val = synthetic()
        D = Sparse(n, n, rowptr, col, val)
        eo = EvenOddDiracOp(D, a.k_synth)
        prob = {"rows": n, "nnz": D.get_nnz(), "ladders": [], "step_cost": []}
        for k in (4, 8):
            ks = [a.k_synth + 0.002 * (j - (k - 1)) for j in range(k)]       # k values up to k_synth, 0.002 apart
            prob["ladders"].append(compare(D, eo, n, ks, 4000, a.runs))
            prob["step_cost"].append(step_cost(D, eo, n, ks, a.runs, 20, 100))
        out["problems"]["synthetic_16x16x16x16x12"] = prob
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
