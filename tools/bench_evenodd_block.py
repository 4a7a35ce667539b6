#!/usr/bin/env python3
"""Even-odd Schur solve of an operator with a dense BLOCK PER SITE (mgcr_eo_create_block) against the full solve, stopped at the same
true residual: GCR(5) from x0 = 0 down to 1e-8 |b| on both sides.

  side A  mgcr_gcr_solve on the full operator DiracOp(D + C, k), tol 1e-8;
  side B  mgcr_eo_solve (EvenOddBlockDiracOp.solve: prepare, GCR on the Schur system of the even half, reconstruct) with
          tol 1e-8 |b| / |bhat_e| — the Schur history is relative to |bhat_e| and the full system's true residual is
          hist[last] |bhat_e| / |b| (include/mgcr.h).

Problems: the 3072-row sample (--sample FILE: text CSR, plain or .gz) with seeded Hermitian 12 x 12 blocks of scale 1 at k = 0.15,
and the periodic 16^4 x 12 lattice of tools/bench_evenodd.py with seeded Hermitian 12 x 12 blocks of scale --scale-synth at
k = --k-synth.  C_s = scale (G + G^H) / 2, G uniform in [-1, 1) + i [-1, 1); a row stores its 12 block entries first.  The sides
ALTERNATE in one process, --runs (>= 6) timings each after one untimed pass; medians and ranges, `ranges_overlap` says where no
claim can be made.  Per side: steps, wall time per solve (host clock around the call, device idle before and after), wall time /
steps, and the true residual |A x - b| / |b| of the LAST solve, computed on the device through the full operator.

Step cost: tol-0 solves at two step caps n1 < n2, per-step cost = (t(n2) - t(n1)) / (n2 - n1), for the full solve through
mgcr_gcr_solve, for the block Schur solve, and for the SITE-DIAGONAL Schur solve (mgcr_eo_create_diag) of the same hopping matrix
with a twisted diagonal +- 0.3 i / k: the block step over the site-diagonal step is the ratio the byte model must explain.
The Schur apply alone (mgcr_bench_op_apply, device events, 20 applies) against its byte model (site blocks), with
V = 16 B per entry and M the stored bytes of both halves: plain apply M + 3 V_e + 2 V_o; site diagonal M + 4 V_e + 3 V_o; site
blocks M + 5 V_e + 4 V_o + 16 bs (n_e + n_o) — the two block streams and the two extra passes (blk_mul_kernel reads and writes an odd
vector, blk_combine_kernel's operand v is written by the SpMV and read back).
One JSON line to stdout; --out FILE (default profiles/evenodd_block.json) writes it too.  No torch import."""
import argparse
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mgpreconditionedgcr_amd import DiracOp, EvenOddBlockDiracOp, EvenOddDiagDiracOp, Field, GCR_Param, Sparse, _lib  # noqa: E402
from bench_evenodd import overlap, solve_call, stats, synthetic, wall_ms  # noqa: E402

RESTART, TOL, BS = 5, 1e-8, 12


def load_text_csr(path):
    """`nrow ncol nnz`, the row offsets, then `col (re,im)` per entry"""
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        nrow, ncol, nnz = (int(t) for t in f.readline().split())
        rowptr = np.empty(nrow + 1, np.int64)
        rowptr[:nrow] = np.array(f.readline().split(), dtype=np.int64)
        rowptr[nrow] = nnz
        body = f.read().replace("(", " ").replace(")", " ").replace(",", " ").split()
    tab = np.array(body[: 3 * nnz], dtype=np.float64).reshape(nnz, 3)
    return nrow, rowptr, tab[:, 0].astype(np.int64), (tab[:, 1] + 1j * tab[:, 2]).astype(np.complex128)


def with_row_heads(n, rowptr, col, val, head_col, head_val):
    """every row gets head_col[r, :] / head_val[r, :] stored in front of its entries"""
    w = head_col.shape[1]
    lens = np.diff(rowptr)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens + w, out=ptr[1:])
    ncol, nval = np.empty(ptr[-1], np.int64), np.empty(ptr[-1], np.complex128)
    head = (ptr[:-1, None] + np.arange(w)[None]).ravel()
    ncol[head], nval[head] = head_col.ravel(), head_val.ravel()
    rows = np.repeat(np.arange(n), lens)
    tail = ptr[rows] + w + (np.arange(col.size) - rowptr[rows])
    ncol[tail], nval[tail] = col, val
    return ptr, ncol, nval


def with_blocks(n, rowptr, col, val, scale, seed=11):
    rng = np.random.default_rng(seed)
    ns = n // BS
    g = rng.uniform(-1, 1, (ns, BS, BS)) + 1j * rng.uniform(-1, 1, (ns, BS, BS))
    blocks = scale * (g + np.conj(np.swapaxes(g, 1, 2))) / 2
    head_col = (np.arange(n) // BS * BS)[:, None] + np.arange(BS)[None]
    return with_row_heads(n, rowptr, col, val, head_col, blocks.reshape(n, BS))


def with_twisted_diagonal(n, rowptr, col, val, k):
    d = np.where(np.arange(n) % 2 == 0, 0.3j, -0.3j) / k
    return with_row_heads(n, rowptr, col, val, np.arange(n)[:, None], d[:, None])


def true_residual(full, b, x):
    r = full(x)
    return float(np.sqrt(b.add_scaled(-1.0, r).squarednorm() / b.squarednorm()))


def per_step(times, n1, n2):
    s1, s2 = stats(times[n1]), stats(times[n2])
    return {"us_per_step": 1e3 * (s2["median"] - s1["median"]) / (n2 - n1), "ms_n1": s1, "ms_n2": s2,
            "us_per_step_range": [1e3 * (s2["min"] - s1["max"]) / (n2 - n1), 1e3 * (s2["max"] - s1["min"]) / (n2 - n1)]}


def step_costs(sides, n, runs, n1, n2):
    """sides: {name: callable(b, x, prm)}; tol 0, the caps and the sides alternating"""
    b, x = Field((n,)).fill_rhs(1), Field((n,))
    prm = {m: GCR_Param(0, RESTART, m, 0.0, False, check_every=50) for m in (n1, n2)}
    t = {name: {n1: [], n2: []} for name in sides}
    for r in range(runs + 1):
        for m in (n1, n2):
            for name, fn in sides.items():
                x.set_zero()
                ms = wall_ms(lambda: fn(b, x, prm[m]))
                if r:
                    t[name][m].append(ms)
    return {name: per_step(t[name], n1, n2) for name in sides}


def apply_model(eo, kind):
    h_eo, h_oe = eo.halves()
    ne, no = eo.sizes()[1:]
    m = h_eo.stored_bytes()["matrix_bytes"] + h_oe.stored_bytes()["matrix_bytes"]
    if kind == "block":
        return m + 16.0 * (5 * ne + 4 * no) + 16.0 * BS * (ne + no)
    return m + 16.0 * (4 * ne + 3 * no)


def bench_apply(eo, kind):
    ne = eo.sizes()[1]
    xe, ye = Field((ne,)).fill_rhs(2), Field((ne,))
    ms = eo.bench_apply(xe, ye, 20)
    model = apply_model(eo, kind)
    return {"us": 1e3 * ms, "byte_model": model, "model_gb_per_s": model / (1e6 * ms)}


def compare(name, n, rowptr, col, val, k, scale, runs, cap, caps):
    M = Sparse(n, n, *with_blocks(n, rowptr, col, val, scale))
    full, eo = DiracOp(M, k), EvenOddBlockDiracOp(M, k, BS)
    Md = Sparse(n, n, *with_twisted_diagonal(n, rowptr, col, val, k))
    eod = EvenOddDiagDiracOp(Md, k)
    b, x = Field((n,)).fill_rhs(1), Field((n,))
    bnorm = float(np.sqrt(b.squarednorm()))
    bhat_norm = float(np.sqrt(eo.prepare(b).squarednorm()))
    prm_a = GCR_Param(0, RESTART, cap, TOL, False, check_every=50)
    prm_b = GCR_Param(0, RESTART, cap, TOL * bnorm / bhat_norm, False, check_every=50)
    a = solve_call(full, prm_a, b, x.set_zero(), cap + 1)             # untimed pass of each side
    eo.solve(b, x.set_zero(), prm_b)
    print("%s: full %d steps (converged %s), even-odd %d steps (converged %s)" % (name, a[0], a[1], eo.last_iterations, eo.last_converged),
          file=sys.stderr, flush=True)
    t_a, t_b = [], []
    for _ in range(runs):
        x.set_zero()
        t_a.append(wall_ms(lambda: solve_call(full, prm_a, b, x, cap + 1)))
        res_a = true_residual(full, b, x)
        x.set_zero()
        t_b.append(wall_ms(lambda: eo.solve(b, x, prm_b)))
        res_b = true_residual(full, b, x)
        print("%s: full %.1f ms, even-odd %.1f ms" % (name, t_a[-1], t_b[-1]), file=sys.stderr, flush=True)
    sa, sb = stats(t_a), stats(t_b)
    eo_steps, eo_conv = eo.last_iterations, eo.last_converged          # (the step-cost solves below overwrite them)
    steps = step_costs({"full": lambda bb, xx, p: solve_call(full, p, bb, xx, p.max_iter + 1),
                        "evenodd_block": lambda bb, xx, p: eo.solve(bb, xx, p),
                        "evenodd_diag": lambda bb, xx, p: eod.solve(bb, xx, p)}, n, runs, *caps)
    ap_b, ap_d = bench_apply(eo, "block"), bench_apply(eod, "diag")
    h_eo, h_oe = eo.halves()
    ne, no = eo.sizes()[1:]
    return {"problem": name, "rows": n, "n_even": ne, "n_odd": no, "bs": BS, "k": k, "block_scale": scale, "tol_true_residual": TOL,
            "schur_tol": TOL * bnorm / bhat_norm,
            "full": {"ms": sa, "steps": a[0], "converged": a[1], "us_per_step": 1e3 * sa["median"] / max(a[0], 1), "true_residual": res_a},
            "evenodd": {"ms": sb, "steps": eo_steps, "converged": eo_conv, "us_per_step": 1e3 * sb["median"] / max(eo_steps, 1),
                        "true_residual": res_b},
            "step_ratio_full_over_evenodd": a[0] / max(eo_steps, 1),
            "wall_ratio_full_over_evenodd": sa["median"] / sb["median"], "ranges_overlap": overlap(sa, sb),
            "step_cost": dict(steps, caps=list(caps),
                              block_over_diag=steps["evenodd_block"]["us_per_step"] / steps["evenodd_diag"]["us_per_step"],
                              block_over_full=steps["evenodd_block"]["us_per_step"] / steps["full"]["us_per_step"]),
            "schur_apply": {"block": ap_b, "site_diagonal": ap_d, "measured_block_over_diag": ap_b["us"] / ap_d["us"],
                            "model_block_over_diag": ap_b["byte_model"] / ap_d["byte_model"]},
            "half_storage": {"H_eo": {"format": h_eo.storage_format()[0], **h_eo.ell_layout()},
                             "H_oe": {"format": h_oe.storage_format()[0], **h_oe.ell_layout()}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", default=os.path.join(ROOT, "tests", "golden", "4x4parsed.txt.gz"), help="the 3072-row sample (text CSR, plain or .gz)")
    ap.add_argument("--parts", nargs="+", default=["sample", "lattice"], choices=["sample", "lattice"])
    ap.add_argument("--k-synth", type=float, default=0.116)
    ap.add_argument("--scale-synth", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--cap", type=int, default=4000, help="step cap of every solve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evenodd_block.json"))
    a = ap.parse_args()
    if a.runs < 6:
        ap.error("--runs must be at least 6")
    import bench
    _lib.init()
    out = {"src_sha16": bench.source_sha16(), "restart": RESTART, "runs": a.runs, "step_cap": a.cap, "cases": []}
    if "sample" in a.parts:
        n, rowptr, col, val = load_text_csr(a.sample)
        out["cases"].append(compare("sample_3072_scale1", n, rowptr, col, val, 0.15, 1.0, a.runs, a.cap, (50, 250)))
    if "lattice" in a.parts:
        n, rowptr, col, val = synthetic()
        out["cases"].append(compare("lattice_16x16x16x16x12", n, rowptr, col, val, a.k_synth, a.scale_synth, a.runs, a.cap, (20, 100)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
