#!/usr/bin/env python3
"""Queued even-odd hopping-parameter scans (EvenOddDiracOp.solve_queue, mgcr_eo_solve_queue) against the two forms an even-odd scan
had before it.  Same right-hand side for every value, GCR(5), tol 1e-10, check_every 50, wall time of the whole ladder.

One JSON line to stdout; --out FILE (default profiles/evenodd_queue.json) writes it too, stamped with the fingerprint of the kernel
sources (bench.source_sha16).  Sides, ALTERNATING in one process, --runs (>= 6) timings each after one untimed pass, medians and
ranges (`ranges_overlap_*` says where no claim can be made):
  A   evenodd_ladder    mgcr_eo_solve per value, mgcr_eo_set_k between them: one k at a time;
  C   evenodd_batched   mgcr_eo_multi_solve; a list of more than 16 values is cut into blocks of 16 in the given order, and every
                        block waits for its slowest column;
  Q2, Q4, Q8            mgcr_eo_solve_queue through 2, 4 and 8 columns.
A and C are the code of the commit before the queue: the yardstick.
Problems:
  (a) the 3072-row sample (--sample FILE, text CSR): the six-value ladder 0.05 .. 0.20 at step cap 4000 (its last value runs many
      times longer than the rest), and 24 values spread evenly over 0.05 .. 0.20;
  (b) the periodic 16^4 x 12 lattice of tools/bench_evenodd.py (786 432 rows): 8 and 24 values up to 0.116, 0.002 apart, cap 4000.
`sum_over_max` = sum of the systems' iteration counts / the largest; `lockstep_steps` = steps the queue launched (mgcr_stat
"eo_queue_steps") and `admissions` = systems loaded after step 0, per call.
`step_cost`: the queue's step is the batched solve's by construction; one pair of tol-0 runs at two step caps on as many values as
columns confirms it: per-step cost = (t(N2) - t(N1)) / (N2 - N1) for C and for Q at the same width.
No torch import."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import EvenOddDiracOp, Field, GCR_Param, MultiEvenOddDiracOp, MultiField, Sparse, _lib, read_data, stat  # noqa: E402
from bench_evenodd import overlap, stats, synthetic, wall_ms  # noqa: E402

RESTART, TOL, CHECK_EVERY = 5, 1e-10, 50
SAMPLE_LADDER = [0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18, 0.20]
WIDTHS = (2, 4, 8)
BLOCK = 16


def sides(eo, n, ks, cap, tol, widths):
    """the ways to run the ladder; each returns the systems' iteration counts.  eo: ONE EvenOddDiracOp per matrix — side A walks it
    with set_k, sides C and Q borrow its halves"""
    nsys = len(ks)
    prm = GCR_Param(0, RESTART, cap, tol, False, check_every=CHECK_EVERY)
    b = Field((n,)).fill_rhs(1)
    x = Field((n,))
    blocks = []
    for g in range(0, nsys, BLOCK):
        part = ks[g:g + BLOCK]
        blocks.append((MultiEvenOddDiracOp(eo, part), MultiField.from_fields([b] * len(part)), MultiField((n,), len(part))))
    xs = [Field((n,)) for _ in ks]

    def ladder():
        its = []
        for kj in ks:
            eo.set_k(kj)
            eo.solve(b, x.set_zero(), prm)
            its.append(eo.last_iterations)
        return its

    def batched():
        its = []
        for scan, B, X in blocks:
            scan.solve(B, X.set_zero(), prm)
            its += list(scan.last_iterations)
        return its

    def queued(width):
        def run():
            for f in xs:
                f.set_zero()
            eo.solve_queue([b] * nsys, xs, ks, prm, width=width)
            return list(eo.last_iterations)
        return run

    fns = {"evenodd_ladder": ladder, "evenodd_batched": batched}
    for w in widths:
        fns["queue_w%d" % w] = queued(w)
    return fns


def timed(fns, runs):
    its, extra, t = {}, {}, {name: [] for name in fns}
    for r in range(runs + 1):
        for name, fn in fns.items():
            box = {}
            before = stat("eo_queue_steps"), stat("eo_queue_admissions")
            ms = wall_ms(lambda: box.update(its=fn()))
            its[name] = box["its"]
            extra[name] = (stat("eo_queue_steps") - before[0], stat("eo_queue_admissions") - before[1])
            if r:
                t[name].append(ms)
    return its, extra, {name: stats(v) for name, v in t.items()}


def compare(eo, n, ks, cap, runs):
    its, extra, ms = timed(sides(eo, n, ks, cap, TOL, WIDTHS), runs)
    ref = its["evenodd_ladder"]
    out = {"ks": [[complex(z).real, complex(z).imag] for z in ks], "step_cap": cap, "iterations": ref,
           "sum_over_max": sum(ref) / max(max(ref), 1),
           "batched_lockstep_steps": sum(max(ref[g:g + BLOCK]) for g in range(0, len(ref), BLOCK))}
    for name in ms:
        assert its[name] == ref, (name, its[name], ref)          # every side runs the same solves
        out[name] = {"ms": ms[name]}
        if name.startswith("queue_"):
            out[name]["lockstep_steps"], out[name]["admissions"] = extra[name]
    for name in ms:
        if not name.startswith("queue_"):
            continue
        for other, key in (("evenodd_ladder", "A"), ("evenodd_batched", "C")):
            out[name]["wall_ratio_%s_over_Q" % key] = ms[other]["median"] / ms[name]["median"]
            out[name]["ranges_overlap_%s" % key] = overlap(ms[other], ms[name])
    return out


def step_cost(eo, n, ks, runs, n1, n2):
    """C and Q at the width of the list, every system to the cap"""
    k = len(ks)
    fns = {m: sides(eo, n, ks, m, 0.0, (k,)) for m in (n1, n2)}
    names = ("evenodd_batched", "queue_w%d" % k)
    t = {(name, m): [] for name in names for m in (n1, n2)}
    for r in range(runs + 1):
        for m in (n1, n2):
            for name in names:
                box = {}
                ms = wall_ms(lambda: box.update(its=fns[m][name]()))
                assert box["its"] == [m] * k, (name, m, box["its"])
                if r:
                    t[(name, m)].append(ms)
    out = {"ks": [[complex(z).real, complex(z).imag] for z in ks], "steps": [n1, n2]}
    for name in names:
        a, c = stats(t[(name, n1)]), stats(t[(name, n2)])
        out[name] = {"ms_at_n1": a, "ms_at_n2": c, "us_per_step": 1e3 * (c["median"] - a["median"]) / (n2 - n1)}
    out["step_ratio_Q_over_C"] = out[names[1]]["us_per_step"] / out[names[0]]["us_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", default=None, help="the 3072-row sample matrix (text CSR, e.g. 4x4parsed.txt); omitted: problem (a) is skipped")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--k-synth", type=float, default=0.116)
    ap.add_argument("--parts", nargs="+", default=["sample", "synthetic"], choices=["sample", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evenodd_queue.json"))
    ap.add_argument("--lib", default=None, help="load this libmgcr_hip.so instead of the in-tree one (one side of a parent / this comparison)")
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import bench
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    _lib.init()
    out = {"src_sha16": bench.source_sha16(), "restart": RESTART, "tol": TOL, "check_every": CHECK_EVERY, "runs": a.runs, "problems": {}}
    if "sample" in a.parts and a.sample:
        D = read_data(os.path.basename(a.sample), directory=os.path.dirname(os.path.abspath(a.sample)))
        n = D.get_dim()
        eo = EvenOddDiracOp(D, SAMPLE_LADDER[0])
        ks24 = [0.05 + 0.15 * j / 23 for j in range(24)]
        out["problems"]["sample"] = {"rows": n, "nnz": D.get_nnz(),
                                     "ladders": [compare(eo, n, SAMPLE_LADDER, 4000, a.runs), compare(eo, n, ks24, 4000, a.runs)],
                                     "step_cost": step_cost(eo, n, [0.13 + 0.004 * j for j in range(8)], a.runs, 50, 250)}
    if "synthetic" in a.parts:
        n, rowptr, col, val = synthetic()
        D = Sparse(n, n, rowptr, col, val)
        eo = EvenOddDiracOp(D, a.k_synth)
        prob = {"rows": n, "nnz": D.get_nnz(), "ladders": []}
        for k in (8, 24):
            ks = [a.k_synth + 0.002 * (j - (k - 1)) for j in range(k)]       # k values up to k_synth, 0.002 apart
            prob["ladders"].append(compare(eo, n, ks, 4000, a.runs))
        prob["step_cost"] = step_cost(eo, n, [a.k_synth + 0.002 * (j - 7) for j in range(8)], a.runs, 20, 100)
        out["problems"]["synthetic_16x16x16x16x12"] = prob
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
