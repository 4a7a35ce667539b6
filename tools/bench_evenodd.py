#!/usr/bin/env python3
"""Even-odd preconditioned solve against the full solve: mgcr_eo_solve (EvenOddDiracOp.solve: prepare, GCR on the Schur system
of the even half, reconstruct) against GCR on DiracOp(D, k), same right-hand side, GCR(5), tol 1e-10.

One JSON line to stdout; --out FILE (default profiles/evenodd.json) writes it too, stamped with the fingerprint of the kernel
sources (bench.source_sha16).  Problems:
  (a) the 3072-row sample (--sample FILE, text CSR) at k = 0.10, 0.15, 0.18 and 0.20 — whether either solve converges there is
      recorded (step cap 4000);
  (b) a synthetic periodic 16^4 lattice with 12 unknowns per site (786 432 rows, 96 entries per row, random complex link blocks, no
      diagonal) built here; k = --k-synth, chosen so that the full solve takes a few hundred steps (the spectrum of such a D fills
      the disc of radius sqrt(96 * 2/3) = 8: GCR contracts by about 8 k per step).
Three sides per problem and k, ALTERNATING in one process, --runs (>= 6) timings each after one untimed pass, medians and ranges
(`ranges_overlap` says where no claim can be made):
  full_call    mgcr_gcr_solve on DiracOp(D, k) — the comparison asked for.  It makes and frees its solver state, Krylov vectors
               included, inside every call;
  full_object  the same solve through a GCR object (mgcr_gcr_create once, mgcr_gcr_solve_op): the state is kept between calls;
  evenodd      mgcr_eo_solve: the operator keeps its solver state between calls, like the GCR object.
So evenodd against full_object is the comparison at equal footing, full_call shows what the per-call state costs.
Wall time per solve (host clock around the call, device idle before and after), iterations, and wall time / iterations, which is
NOT a step cost: it carries the per-solve part (start, last step, download; prepare, split, reconstruct, merge on the even-odd
side).  The two are separated by `step_cost`: full_object and evenodd with tol 0 at two step caps N1 < N2, per-step cost =
(t(N2) - t(N1)) / (N2 - N1), per-solve cost = t(N1) - N1 x per-step cost (sample: k = 0.15, 50 and 250 steps; lattice: 20 and 100).
Byte model per step next to it (M = bytes of D's stored entries, 20 B each; V = 16 n; both solves run the multi-kernel lean path
here): residual update 3 + apply 2 + beta dots lim + build 3 + lim vectors, 3 + lim more in the step that closes a cycle — 15.6
vectors per step averaged over a GCR(5) cycle.  Full: M + 15.6 V.  Even-odd: the same launches on half-length vectors plus the
write and read of t = D_oe x: M + 15.6 V/2 + 2 V/2 = M + 8.8 V; one launch more per step (two applies).  No torch import."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mgpreconditionedgcr_amd import DiracOp, EvenOddDiracOp, Field, GCR, GCR_Param, Sparse, _lib, read_data  # noqa: E402

RESTART, TOL, CAP = 5, 1e-10, 4000
SAMPLE_KS = [0.10, 0.15, 0.18, 0.20]


def stats(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def wall_ms(fn):
    L = _lib.lib()
    _lib.check(L.mgcr_synchronize())
    t0 = time.perf_counter()
    fn()
    _lib.check(L.mgcr_synchronize())
    return 1e3 * (time.perf_counter() - t0)


def synthetic(dims=(16, 16, 16, 16), ncomp=12, seed=7):
    """Periodic nearest-neighbour hopping matrix, one random complex ncomp x ncomp block per (site, direction, sign); a row's
    entries are stored direction by direction (no sort: 75 M entries)"""
    rng = np.random.default_rng(seed)
    nsite = int(np.prod(dims))
    coords = np.stack(np.unravel_index(np.arange(nsite, dtype=np.int64), dims), axis=1)
    nb = np.empty((nsite, 2 * len(dims)), np.int64)
    for mu in range(len(dims)):
        for s, sign in enumerate((-1, 1)):
            c = coords.copy()
            c[:, mu] = (c[:, mu] + sign) % dims[mu]
            nb[:, 2 * mu + s] = np.ravel_multi_index(tuple(c.T), dims)
    nd = nb.shape[1]
    # col[site, a, dir, b] = nb[site, dir] * ncomp + b
    col = (nb[:, None, :, None] * ncomp + np.arange(ncomp, dtype=np.int64)[None, None, None, :])
    col = np.ascontiguousarray(np.broadcast_to(col, (nsite, ncomp, nd, ncomp))).reshape(-1)
    n = nsite * ncomp
    val = np.empty(col.size, np.complex128)
    val.real = rng.uniform(-1, 1, col.size)
    val.imag = rng.uniform(-1, 1, col.size)
    rowptr = np.arange(n + 1, dtype=np.int64) * (nd * ncomp)
    return n, rowptr, col, val


def solve_call(op, prm, b, x, cap):
    """mgcr_gcr_solve: (iterations, converged, last history entry)"""
    hist = np.zeros(cap, np.float64)
    it, conv = C.c_int32(), C.c_int32()
    pc = prm._c()
    _lib.check(_lib.lib().mgcr_gcr_solve(op.h, C.byref(pc), b.h, x.h, hist.ctypes.data, cap, C.byref(it), C.byref(conv)))
    return it.value, bool(conv.value), float(hist[it.value])


def side(ms, its, conv, res):
    return {"ms": ms, "iterations": its, "converged": conv, "final_residual": res, "wall_us_over_iterations": 1e3 * ms["median"] / max(its, 1)}


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def compare(D, n, k, b, runs):
    prm = GCR_Param(0, RESTART, CAP, TOL, False, check_every=50)
    dirac = DiracOp(D, k)
    full = GCR(dirac, prm)
    eo = EvenOddDiracOp(D, k)
    x = Field((n,))
    call = solve_call(dirac, prm, b, x.set_zero(), CAP + 1)
    full.solve(b, x.set_zero())
    eo.solve(b, x.set_zero(), prm)
    t_call, t_obj, t_eo = [], [], []
    for _ in range(runs):
        x.set_zero()
        t_call.append(wall_ms(lambda: solve_call(dirac, prm, b, x, CAP + 1)))
        x.set_zero()
        t_obj.append(wall_ms(lambda: full.solve(b, x)))
        x.set_zero()
        t_eo.append(wall_ms(lambda: eo.solve(b, x, prm)))
    sc, so, se = stats(t_call), stats(t_obj), stats(t_eo)
    assert call[0] == full.last_iterations
    d_eo, d_oe = eo.halves()
    M, V = 20.0 * D.get_nnz(), 16.0 * n
    return {"k": k, "full_call": side(sc, *call), "full_object": side(so, full.last_iterations, full.last_converged, float(full.last_history[-1])),
            "evenodd": side(se, eo.last_iterations, eo.last_converged, float(eo.last_history[-1])),
            "wall_ratio_full_call_over_evenodd": sc["median"] / se["median"], "ranges_overlap_full_call": overlap(sc, se),
            "wall_ratio_full_object_over_evenodd": so["median"] / se["median"], "ranges_overlap_full_object": overlap(so, se),
            "byte_model": {"full_bytes_per_step": M + 15.6 * V, "evenodd_bytes_per_step": M + 8.8 * V,
                           "per_step_ratio": (M + 15.6 * V) / (M + 8.8 * V)},
            "half_storage": {"D_eo": {"format": d_eo.storage_format()[0], **d_eo.ell_layout()},
                             "D_oe": {"format": d_oe.storage_format()[0], **d_oe.ell_layout()}},
            "full_storage": {"format": D.storage_format()[0], **D.ell_layout()}}


def step_cost(D, n, k, b, runs, n1, n2):
    """per-step and per-solve cost of full_object and evenodd: tol 0, step caps n1 < n2"""
    full = {m: GCR(DiracOp(D, k), GCR_Param(0, RESTART, m, 0.0, False, check_every=50)) for m in (n1, n2)}
    prm = {m: GCR_Param(0, RESTART, m, 0.0, False, check_every=50) for m in (n1, n2)}
    eo = EvenOddDiracOp(D, k)
    x = Field((n,))
    t = {("full", n1): [], ("full", n2): [], ("eo", n1): [], ("eo", n2): []}
    for r in range(runs + 1):
        for m in (n1, n2):
            x.set_zero()
            tf = wall_ms(lambda: full[m].solve(b, x))
            x.set_zero()
            te = wall_ms(lambda: eo.solve(b, x, prm[m]))
            assert full[m].last_iterations == m and eo.last_iterations == m
            if r:
                t[("full", m)].append(tf)
                t[("eo", m)].append(te)
    out = {"k": k, "steps": [n1, n2]}
    for name in ("full", "eo"):
        a, c = stats(t[(name, n1)]), stats(t[(name, n2)])
        per_step = (c["median"] - a["median"]) / (n2 - n1)
        out["full_object" if name == "full" else "evenodd"] = {"ms_at_n1": a, "ms_at_n2": c, "us_per_step": 1e3 * per_step,
                                                                "us_per_solve": 1e3 * (a["median"] - n1 * per_step)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", default=None, help="the 3072-row sample matrix (text CSR, e.g. 4x4parsed.txt); omitted: problem (a) is skipped")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--k-synth", type=float, default=0.116)
    ap.add_argument("--parts", nargs="+", default=["sample", "synthetic"], choices=["sample", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evenodd.json"))
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import bench
    _lib.init()
    out = {"src_sha16": bench.source_sha16(), "restart": RESTART, "tol": TOL, "step_cap": CAP, "runs": a.runs, "problems": {}}
    if "sample" in a.parts and a.sample:
        D = read_data(os.path.basename(a.sample), directory=os.path.dirname(os.path.abspath(a.sample)))
        n = D.get_dim()
        b = Field((n,)).fill_rhs(1)
        out["problems"]["sample"] = {"rows": n, "nnz": D.get_nnz(), "cases": [compare(D, n, k, b, a.runs) for k in SAMPLE_KS],
                                     "step_cost": step_cost(D, n, 0.15, b, a.runs, 50, 250)}
    if "synthetic" in a.parts:
        n, rowptr, col, val = synthetic()
        D = Sparse(n, n, rowptr, col, val)
        b = Field((n,)).fill_rhs(1)
        out["problems"]["synthetic_16x16x16x16x12"] = {"rows": n, "nnz": D.get_nnz(), "cases": [compare(D, n, a.k_synth, b, a.runs)],
                                                         "step_cost": step_cost(D, n, a.k_synth, b, a.runs, 20, 100)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
