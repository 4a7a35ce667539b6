#!/usr/bin/env python3
"""Multi-RHS measurement: the k-wide apply against k single applies, the batched GCR against k single solves.

One JSON line to stdout (--out FILE writes it too).  For k in --ks (default 1 2 4 8 12):
  1. block-CSR, bs 20, 36 000 block rows (problems.unstructured_blocks): apply_multi(k) against k x apply;
  2. irregular CSR, 8 Mi rows (problems.skewed_csr), windows 2^17 and 900, cold caches (a 256 MiB -> 256 MiB copy sweeps the caches before every timed apply);
  3. GCR(5), Poisson 128^3, 20 steps, tol 0: solve_multi(k) against k single solves (system-iterations per second).
Every figure is the median of --runs (>= 6) timings with the two sides interleaved (A B A B ...), range reported; hipEvents on
the library stream (mgcr_timer_*, mgcr_bench_op_apply, mgcr_bench_op_apply_multi).
  4. (--parts kscan, not in the default set; result also written to profiles/kscan.json with --out) hopping-parameter scans, one
     MultiDiracOp solve against one DiracOp solve per value, on (a) the 3072-row sample (--sample FILE, text CSR) and (b) a DiracOp on
     problems.skewed_csr with 2^20 rows and window 2^17: equal-length columns (k = 4, 8, tol 0, 200 steps on (a), 40 on (b); time per
     system-iteration), and the six-value scan of tests/kscan_cases.py on (a) (batched wall time against the sum of the six single
     solves: the batched solve runs as long as its slowest column);
  5. (--parts uniform --lib SO: one side; --parts uniform_ab --parent-lib SO: both sides, alternating, one process per timing)
     apply_multi of a plain DiracOp at k = 8 on (a) and (b) with the library of the parent commit against this one, next to the spread
     of parent against parent from the same call.  Next to each measured ratio stands the
  6. (--parts queue, not in the default set; profiles/queue.json with --out) the queued solve (GCR.solve_queue): the six-value scan on
     (a) as six DiracOp solves, as one solve_multi at k = 6 and as solve_queue at W = 2, 3, 4 in the given order and longest first — wall
     time, lockstep steps (mgcr_stat "queue_steps"), microseconds per lockstep step — next to the schedule's model; and on (b) six
     shifts 0.010 .. 0.050 capped at 40 steps with ONE tolerance (a call takes one) taken from a first pass, between the third and
     the fourth column's final residual, so that the stops differ.  --parts kscan_ab --parent-lib SO:
     the existing batched solve (the scan and the equal-length k = 8 solve on (a), --parts kscan_side) with the parent commit's
     library against this one, alternating processes, next to the parent's own spread.
byte-model ratio k (M + 2 V) / (M + 2 k V), M = matrix bytes, V = 16 n; for the solve, bytes per step from the terms of
bench.py's gcr_phase_model, averaged over a GCR(5) cycle (lim = 1 .. 5 stored directions): the single solve's one-launch steps
move M + (2 lim + 4) V in a cycle and M + (3 R + 5) V in the step that closes it (11.2 V on average); the batched solve moves,
per system, 3 V (residual update) + 2 V (apply) + (lim + ceil(lim / 2)) V (beta dots, two directions per pass) + (3 + lim) V
(build) and (3 + lim) V more in the closing step (17.4 V on average), and M once per step.  No torch import."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgpreconditionedgcr_amd import (DiracOp, Field, GCR, GCR_Param, HierarchicalSparse, MultiField, Sparse, _lib, problems,  # noqa: E402
                                     read_data)


def stats(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def timer(fn):
    L = _lib.lib()
    _lib.check(L.mgcr_timer_start())
    fn()
    ms = C.c_double()
    _lib.check(L.mgcr_timer_stop(C.byref(ms)))
    return ms.value


def apply_pair(A, n, k, runs, reps, cold):
    """(k x single apply, apply_multi(k)) in ms, interleaved; cold: one apply per timing behind a cache-flushing sweep"""
    f = [Field((n,)).fill_rhs(j) for j in range(k)]
    y = Field((n,))
    X = MultiField.from_fields(f)
    Y = MultiField((n,), k)
    # cold: a 256 MiB -> 256 MiB copy sweeps L2 and the Infinity Cache in front of every timed apply
    sweep_a, sweep_b = (Field((1 << 24,)).set_zero(), Field((1 << 24,))) if cold else (None, None)
    single, multi = [], []
    A(f[0], out=y)
    A.apply_multi(X, out=Y)
    for _ in range(runs):
        if cold:
            t = 0.0
            for j in range(k):
                sweep_b.assign(sweep_a)
                t += timer(lambda: A(f[j], out=y))
            single.append(t)
            sweep_b.assign(sweep_a)
            multi.append(timer(lambda: A.apply_multi(X, out=Y)))
        else:
            single.append(sum(A.bench_apply(f[j], y, reps=reps) for j in range(k)))
            multi.append(A.bench_apply_multi(X, Y, reps=reps))
    return stats(single), stats(multi)


def record(k, s, m, M, V):
    return {"k": k, "single_ms": s, "multi_ms": m, "ratio": s["median"] / m["median"],
            "ranges_overlap": not (m["max"] < s["min"] or s["max"] < m["min"]),
            "byte_model_ratio": k * (M + 2 * V) / (M + 2 * k * V)}


SCAN_KS = [0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18, 0.20]      # tests/kscan_cases.py
SCAN_ARGS = (0, 5, 400, 1e-10)


def kscan_systems(sample):
    n = 1 << 20
    yield "sample", read_data(os.path.basename(sample), directory=os.path.dirname(os.path.abspath(sample))), 200, \
        lambda k: [0.05 + 0.13 * j / (k - 1) for j in range(k)]
    yield "skewed_2p20_w2p17", Sparse(n, n, *problems.skewed_csr(n, np.random.default_rng(4), window=1 << 17)), 40, \
        lambda k: [0.01 + 0.002 * j for j in range(k)]


def scan_pair(D, ks, args, rhs, runs):
    """(one single solve per k_j, one batched solve with per-column k) in ms, interleaved; iterations per column of either side"""
    from mgpreconditionedgcr_amd import MultiDiracOp
    n, k = D.get_dim(), len(ks)
    prm = GCR_Param(*args, False)
    singles = [GCR(DiracOp(D, kj), prm) for kj in ks]
    gm = GCR(MultiDiracOp(D, ks), prm)
    x, X = Field((n,)), MultiField((n,), k)
    R = MultiField.from_fields(rhs)
    for j in range(k):
        singles[j].solve(rhs[j], x.set_zero())
    gm.solve_multi(R, X.set_zero())
    its_single, its_multi = [g.last_iterations for g in singles], list(gm.last_iterations)
    finite = all(np.isfinite(h).all() for h in gm.last_history)
    single, multi = [], []
    for _ in range(runs):
        t = 0.0
        for j in range(k):
            x.set_zero()
            t += timer(lambda: singles[j].solve(rhs[j], x))
        single.append(t)
        X.set_zero()
        multi.append(timer(lambda: gm.solve_multi(R, X)))
    return stats(single), stats(multi), its_single, its_multi, finite


def kscan(sample, runs):
    out = {}
    for name, D, steps, ladder in kscan_systems(sample):
        n = D.get_dim()
        rec = {"rows": n, "layout": D.ell_layout(), "storage_format": D.storage_format()[0], "steps": steps, "restart": 5, "equal_length": []}
        b = Field((n,)).fill_rhs(1)
        for k in (4, 8):
            s, m, its_s, its_m, finite = scan_pair(D, ladder(k), (0, 5, steps, 0.0), [b] * k, runs)
            assert its_s == its_m == [steps] * k, (its_s, its_m)
            rec["equal_length"].append({"k": k, "ks": [str(v) for v in ladder(k)], "single_ms": s, "multi_ms": m, "histories_finite": finite,
                                        "ratio": s["median"] / m["median"],
                                        "ranges_overlap": not (m["max"] < s["min"] or s["max"] < m["min"]),
                                        "single_us_per_system_iteration": 1e3 * s["median"] / (k * steps),
                                        "multi_us_per_system_iteration": 1e3 * m["median"] / (k * steps)})
        if name == "sample":
            b = Field((n,), problems.rhs_grid(n, 1))
            s, m, its_s, its_m, _ = scan_pair(D, SCAN_KS, SCAN_ARGS, [b] * len(SCAN_KS), runs)
            assert its_s == its_m, (its_s, its_m)
            rec["scan"] = {"ks": [str(v) for v in SCAN_KS], "restart": 5, "max_iter": 400, "tol": 1e-10, "iterations": its_m,
                           "sum_of_singles_ms": s, "batched_ms": m, "ratio_singles_over_batched": s["median"] / m["median"],
                           "ranges_overlap": not (m["max"] < s["min"] or s["max"] < m["min"]),
                           "sum_iterations": sum(its_m), "max_iterations": max(its_m),
                           "batched_us_per_lockstep_step": 1e3 * m["median"] / max(its_m),
                           "single_us_per_iteration": 1e3 * s["median"] / sum(its_m)}
        out[name] = rec
        del D
    return out


def uniform_side(sample, runs):
    """apply_multi of a plain DiracOp at k = 8 (the uniform-shift path), ms per apply, on the two systems of the scan measurement"""
    out = {}
    for name, D, _, _ in kscan_systems(sample):
        n = D.get_dim()
        A = DiracOp(D, 0.15 + 0.05j)
        X = MultiField.from_fields([Field((n,)).fill_rhs(j) for j in range(8)])
        Y = MultiField((n,), 8)
        reps = 2000 if n < 1 << 16 else 40
        A.bench_apply_multi(X, Y, reps=reps)
        out[name] = stats([A.bench_apply_multi(X, Y, reps=reps) for _ in range(runs)])
        out[name]["checksum"] = float(Y.squarednorm().sum())
    return out


def uniform_ab(sample, parent_lib, runs):
    """parent, this, parent, this, ...: one process per timing (a process loads one library); the spread of parent against parent is
    the spread between the parent's own processes"""
    import subprocess
    sides = {"parent": [], "this": []}
    for _ in range(runs):
        for side, lib in (("parent", parent_lib), ("this", _lib.LIB_PATH)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parts", "uniform", "--lib", lib, "--sample", sample],
                               capture_output=True, text=True, check=True, timeout=600)
            sides[side].append(json.loads(p.stdout.strip().splitlines()[-1])["uniform"])
    out = {}
    for name in sides["parent"][0]:
        pa = [r[name]["median"] for r in sides["parent"]]
        th = [r[name]["median"] for r in sides["this"]]
        assert len({r[name]["checksum"] for r in sides["parent"] + sides["this"]}) == 1      # the same bits from both libraries
        out[name] = {"k": 8, "parent_ms": stats(pa), "this_ms": stats(th), "this_over_parent": float(np.median(th) / np.median(pa)),
                     "parent_spread": (max(pa) - min(pa)) / float(np.median(pa)),
                     "inside_parent_spread": bool(min(pa) <= np.median(th) <= max(pa))}
    return out


from tests.queue_cases import LONGEST_FIRST_KS as LONGEST_FIRST, lockstep_steps  # noqa: E402  (the schedule's model the tests assert)


def queue_sides(D, b, ks, args, widths, runs, orders):
    """interleaved: the single solves, one solve_multi over all of ks, solve_queue per (order, W); ms, iterations, lockstep steps"""
    from mgpreconditionedgcr_amd import MultiDiracOp, stat
    n, k = D.get_dim(), len(ks)
    prm = GCR_Param(*args, False, check_every=args[1])
    singles = [GCR(DiracOp(D, kj), prm) for kj in ks]
    gm, gq = GCR(MultiDiracOp(D, ks), prm), GCR(D, prm)
    x, X, xs = Field((n,)), MultiField((n,), k), [Field((n,)) for _ in ks]
    R = MultiField.from_fields([b] * k)
    for j in range(k):
        singles[j].solve(b, x.set_zero())
    its = [g.last_iterations for g in singles]
    gm.solve_multi(R, X.set_zero())
    assert list(gm.last_iterations) == its
    conf = [(name, order, W) for name, order in orders for W in widths]
    steps = {}
    for name, order, W in conf:
        for f in xs:
            f.set_zero()
        before = stat("queue_steps")
        gq.solve_queue([b] * k, xs, width=W, ks=order)
        steps[(name, W)] = stat("queue_steps") - before
        assert sorted(gq.last_iterations) == sorted(its)
    t_single, t_multi, t_queue = [], [], {c[0::2]: [] for c in conf}
    for _ in range(runs):
        t = 0.0
        for j in range(k):
            x.set_zero()
            t += timer(lambda: singles[j].solve(b, x))
        t_single.append(t)
        X.set_zero()
        t_multi.append(timer(lambda: gm.solve_multi(R, X)))
        for name, order, W in conf:
            for f in xs:
                f.set_zero()
            t_queue[(name, W)].append(timer(lambda: gq.solve_queue([b] * k, xs, width=W, ks=order)))
    s, m = stats(t_single), stats(t_multi)
    rec = {"ks": [str(v) for v in ks], "restart": args[1], "max_iter": args[2], "tol": args[3], "iterations": its, "sum_iterations": sum(its),
           "singles_ms": s, "single_us_per_iteration": 1e3 * s["median"] / sum(its),
           "batched_ms": m, "batched_lockstep_steps": max(its), "batched_us_per_lockstep_step": 1e3 * m["median"] / max(its),
           "singles_over_batched": s["median"] / m["median"], "queue": []}
    for name, order, W in conf:
        q = stats(t_queue[(name, W)])
        order_its = [its[ks.index(v)] for v in order]
        rec["queue"].append({"order": name, "width": W, "ms": q, "lockstep_steps": steps[(name, W)],
                             "model_lockstep_steps": lockstep_steps(order_its, W, args[1]),
                             "us_per_lockstep_step": 1e3 * q["median"] / steps[(name, W)],
                             "singles_over_queue": s["median"] / q["median"], "batched_over_queue": m["median"] / q["median"],
                             "ranges_overlap_singles": not (q["max"] < s["min"] or s["max"] < q["min"]),
                             "ranges_overlap_batched": not (q["max"] < m["min"] or m["max"] < q["min"])})
    return rec


def queue_part(sample, runs, large=True):
    out = {}
    D = read_data(os.path.basename(sample), directory=os.path.dirname(os.path.abspath(sample)))
    n = D.get_dim()
    out["sample"] = dict(rows=n, **queue_sides(D, Field((n,), problems.rhs_grid(n, 1)), SCAN_KS, SCAN_ARGS, (2, 3, 4), runs,
                                               [("given", SCAN_KS), ("longest_first", LONGEST_FIRST)]))
    del D
    if large:      # the matrix stream dominates a step: 2^20 rows
        n = 1 << 20
        D = Sparse(n, n, *problems.skewed_csr(n, np.random.default_rng(4), window=1 << 17))
        b = Field((n,)).fill_rhs(1)
        for spacing in (0.008, 0.002):      # wider than the kscan part's ladder (0.002) so that the columns' rates differ — if all of it converges
            ks = [0.01 + spacing * j for j in range(6)]
            hist = []
            for kj in ks:      # first pass: 40 steps each, then ONE tolerance for the call (the entry point takes one)
                g = GCR(DiracOp(D, kj), GCR_Param(0, 5, 40, 0.0, False))
                g.solve(b, Field((n,)).set_zero())
                hist.append(g.last_history)
            ends = sorted(float(h[-1]) for h in hist)
            if np.isfinite(ends).all() and ends[-1] < 1e-2:
                break
        tol = float(np.sqrt(ends[2] * ends[3]))      # between the third and the fourth column's: three stop early, at their own steps
        out["skewed_2p20_w2p17"] = dict(rows=n, first_pass_final_residuals=ends,
                                        **queue_sides(D, b, ks, (0, 5, 40, tol), (2, 3, 4), runs, [("given", ks), ("longest_first", ks[::-1])]))
    return out


def kscan_side(sample, runs):
    """the existing batched solve on the sample: the six-value scan and the equal-length k = 8 solve (ms), one side of kscan_ab"""
    from mgpreconditionedgcr_amd import MultiDiracOp
    D = read_data(os.path.basename(sample), directory=os.path.dirname(os.path.abspath(sample)))
    n = D.get_dim()
    out = {}
    for name, ks, args, b in (("scan", SCAN_KS, SCAN_ARGS, Field((n,), problems.rhs_grid(n, 1))),
                              ("equal_k8", [0.05 + 0.13 * j / 7 for j in range(8)], (0, 5, 200, 0.0), Field((n,)).fill_rhs(1))):
        g = GCR(MultiDiracOp(D, ks), GCR_Param(*args, False))
        R, X = MultiField.from_fields([b] * len(ks)), MultiField((n,), len(ks))
        g.solve_multi(R, X.set_zero())
        t = []
        for _ in range(runs):
            X.set_zero()
            t.append(timer(lambda: g.solve_multi(R, X)))
        out[name] = stats(t)
        out[name]["checksum"] = float(X.squarednorm().sum())
        out[name]["iterations"] = list(g.last_iterations)
    return out


def kscan_ab(sample, parent_lib, runs):
    """uniform_ab's protocol for the batched solve: parent, this, parent, this, ... one process per timing"""
    import subprocess
    sides = {"parent": [], "this": []}
    for _ in range(runs):
        for side, lib in (("parent", parent_lib), ("this", _lib.LIB_PATH)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parts", "kscan_side", "--lib", lib, "--sample", sample],
                               capture_output=True, text=True, check=True, timeout=600)
            sides[side].append(json.loads(p.stdout.strip().splitlines()[-1])["kscan_side"])
    out = {}
    for name in sides["parent"][0]:
        pa = [r[name]["median"] for r in sides["parent"]]
        th = [r[name]["median"] for r in sides["this"]]
        assert len({r[name]["checksum"] for r in sides["parent"] + sides["this"]}) == 1      # the same bits from both libraries
        out[name] = {"parent_ms": stats(pa), "this_ms": stats(th), "this_over_parent": float(np.median(th) / np.median(pa)),
                     "parent_spread": (max(pa) - min(pa)) / float(np.median(pa)),
                     "inside_parent_spread": bool(min(pa) <= np.median(th) <= max(pa))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8, 12])
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--parts", nargs="+", default=["bcsr", "irregular", "gcr"])
    ap.add_argument("--block-rows", type=int, default=36000)
    ap.add_argument("--irregular-rows", type=int, default=1 << 23)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", default=None, help="kscan / uniform / queue: the 3072-row sample matrix (text CSR, e.g. 4x4parsed.txt)")
    ap.add_argument("--lib", default=None, help="uniform / kscan_side: load this libmgcr_hip.so instead of the in-tree one")
    ap.add_argument("--parent-lib", default=None, help="uniform_ab / kscan_ab: the library built from the parent commit")
    ap.add_argument("--queue-sample-only", action="store_true", help="queue: leave out the 2^20-row system")
    a = ap.parse_args()
    runs = max(6, a.runs)
    out = {"tool": "bench_multi_rhs", "runs": runs}
    if a.lib:      # (a library from before the MultiDiracOp entry points lacks their symbols: bind what it has)
        _lib.LIB_PATH = os.path.abspath(a.lib)
        have = C.CDLL(_lib.LIB_PATH)
        for name in [nm for nm in _lib._SIGS if not hasattr(have, nm)]:
            del _lib._SIGS[name]
    if "kscan" in a.parts:
        out["kscan"] = kscan(a.sample, runs)
    if "uniform" in a.parts:
        out["uniform"] = uniform_side(a.sample, runs)
    if "queue" in a.parts:
        out["queue"] = queue_part(a.sample, runs, not a.queue_sample_only)
    if "kscan_side" in a.parts:
        out["kscan_side"] = kscan_side(a.sample, runs)
    if "kscan_ab" in a.parts:
        out["kscan_ab"] = kscan_ab(a.sample, a.parent_lib, runs)
    if "uniform_ab" in a.parts:
        out["uniform_ab"] = uniform_ab(a.sample, a.parent_lib, runs)
    if "bcsr" in a.parts:
        nb, bs = a.block_rows, 20
        rows, cols, blocks = problems.unstructured_blocks(nb, bs)
        H = HierarchicalSparse(nb, nb, rows, cols, blocks)
        M, n = H.stored_bytes()["matrix_bytes"], nb * bs
        del blocks
        out["bcsr"] = {"block_rows": nb, "bs": bs, "matrix_bytes": M,
                       "k": [record(k, *apply_pair(H, n, k, runs, 5, False), M, 16 * n) for k in a.ks]}
        del H
    if "irregular" in a.parts:
        n = a.irregular_rows
        for window in (1 << 17, 900):
            A = Sparse(n, n, *problems.skewed_csr(n, np.random.default_rng(4), window=window))
            M = A.stored_bytes()["matrix_bytes"]
            out["irregular_w%d" % window] = {"rows": n, "window": window, "matrix_bytes": M, "layout": A.ell_layout(),
                                             "k": [record(k, *apply_pair(A, n, k, runs, 1, True), M, 16 * n) for k in a.ks]}
            del A
    if "gcr" in a.parts:
        nn, steps = 128, 20
        lims = [1, 2, 3, 4, 5]
        v_single = sum((2 * l + 4) if l < 5 else 20 for l in lims) / 5.0
        v_multi = sum(3 + 2 + l + (l + 1) // 2 + (3 + l) + ((3 + l) if l == 5 else 0) for l in lims) / 5.0
        A = Sparse(*problems.poisson3d_csr(nn))
        n = nn ** 3
        M, V = A.stored_bytes()["matrix_bytes"], 16 * n
        prm = GCR_Param(0, 5, steps, 0.0, False)
        recs = []
        for k in a.ks:
            rhs = [Field((n,)).fill_rhs(1 + j) for j in range(k)]
            x = Field((n,))
            R, X = MultiField.from_fields(rhs), MultiField((n,), k)
            gs, gm = GCR(A, prm), GCR(A, prm)
            gs.solve(rhs[0], x.set_zero())
            gm.solve_multi(R, X.set_zero())
            single, multi = [], []
            for _ in range(runs):
                t = 0.0
                for j in range(k):
                    x.set_zero()
                    t += timer(lambda: gs.solve(rhs[j], x))
                single.append(t)
                X.set_zero()
                multi.append(timer(lambda: gm.solve_multi(R, X)))
            s, m = stats(single), stats(multi)
            recs.append({"k": k, "single_ms": s, "multi_ms": m, "ratio": s["median"] / m["median"],
                         "ranges_overlap": not (m["max"] < s["min"] or s["max"] < m["min"]),
                         "single_system_it_per_s": k * steps / s["median"] * 1e3, "multi_system_it_per_s": k * steps / m["median"] * 1e3,
                         "byte_model_ratio": k * (M + v_single * V) / (M + k * v_multi * V)})
        out["gcr_poisson128"] = {"n": nn, "steps": steps, "restart": 5, "k": recs}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
