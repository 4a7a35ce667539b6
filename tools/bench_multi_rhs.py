#!/usr/bin/env python3
"""Multi-RHS measurement: the k-wide apply against k single applies, the batched GCR against k single solves.

One JSON line to stdout (--out FILE writes it too).  For k in --ks (default 1 2 4 8 12):
  1. block-CSR, bs 20, 36 000 block rows (problems.unstructured_blocks): apply_multi(k) against k x apply;
  2. irregular CSR, 8 Mi rows (problems.skewed_csr), windows 2^17 and 900, cold caches (a 256 MiB -> 256 MiB copy sweeps the caches before every timed apply);
  3. GCR(5), Poisson 128^3, 20 steps, tol 0: solve_multi(k) against k single solves (system-iterations per second).
Every figure is the median of --runs (>= 6) timings with the two sides interleaved (A B A B ...), range reported; hipEvents on
the library stream (mgcr_timer_*, mgcr_bench_op_apply, mgcr_bench_op_apply_multi).  Next to each measured ratio stands the
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
from mgpreconditionedgcr_amd import (Field, GCR, GCR_Param, HierarchicalSparse, MultiField, Sparse, _lib, problems)  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8, 12])
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--parts", nargs="+", default=["bcsr", "irregular", "gcr"])
    ap.add_argument("--block-rows", type=int, default=36000)
    ap.add_argument("--irregular-rows", type=int, default=1 << 23)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runs = max(6, a.runs)
    out = {"tool": "bench_multi_rhs", "runs": runs}
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
