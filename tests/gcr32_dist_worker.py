"""Worker of tests/test_gpu_gcr32.py::test_rule_d_a_distributed_outer_operator_is_refused (a plain script, like tests/dist_worker.py):
    gcr32_dist_worker.py RANK WORLD PORT OUTDIR
Every rank holds a row block of case (d)'s hopping matrix as a DistSparse and the plain and the Dirac form of it as outer operators,
and a LowPrecisionGCR of the whole matrix; it puts the latter into right_precond (flexible = 1) of mgcr_gcr_solve, mgcr_gcr_create
and mgcr_gcr_set_operator on the distributed operators and saves (code, message) of each refusal as OUTDIR/rankR.json."""
import ctypes as C
import json
import os
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Comm, DiracOp, DistSparse, Field, GCR, GCR_Param, LowPrecisionGCR, MgcrError, _lib
    from tests import gcr32_cases as g
    from tests.dist_worker import local_block
    comm = Comm.host(dist)
    mg.init(0)
    c = g.case("d")
    per = c.n // world
    r0, r1 = rank * per, (rank + 1) * per
    lp, lc, lv = local_block(c.rowptr, c.col, c.val, r0, r1)
    A0 = DistSparse(comm, c.n, r0, lp, lc, lv)
    A = DiracOp(A0, c.k)
    # the fp32 copy of the local diagonal block would be the natural candidate: rows r0 .. r1, columns outside dropped
    keep = (lc >= r0) & (lc < r1)
    import numpy as np
    rows = np.repeat(np.arange(r1 - r0), np.diff(lp))[keep]
    rp = np.zeros(r1 - r0 + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=r1 - r0), out=rp[1:])
    local = types.SimpleNamespace(ROW=rp, COL=np.ascontiguousarray(lc[keep] - r0, np.int64), VAL=np.ascontiguousarray(lv[keep], np.complex128))
    low = LowPrecisionGCR(local, c.k, GCR_Param(0, 8, 8, 0.1, False))
    good = GCR_Param(0, 5, 50, 1e-10, False, solver_r=low, flexible=True)
    b, x = Field((r1 - r0,), g.rhs(c.n)[r0:r1]), Field((r1 - r0,)).set_zero()
    out = {}

    def refused(where, fn):
        try:
            fn()
            out[where] = (0, "accepted")
        except MgcrError as e:
            out[where] = (e.code, str(e))

    def solve(M):
        pc = good._c()
        _lib.check(_lib.lib().mgcr_gcr_solve(M.h, C.byref(pc), b.h, x.h, None, 0, None, None))

    refused("solve_sparse", lambda: solve(A0))
    refused("solve_dirac", lambda: solve(A))
    refused("create_sparse", lambda: GCR(A0, good))
    refused("create_dirac", lambda: GCR(A, good))
    refused("set_operator", lambda: GCR(good).initialise(A))
    with open(os.path.join(outdir, "rank%d.json" % rank), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
