#!/usr/bin/env python3
"""bench.py — headline benchmark of the hot path: restarted GCR iterations/sec on the 3-D 7-point Poisson system of
BASELINE.json configs[1] (128^3, unpreconditioned GCR restart 5, complex fp64, x0 = 0, deterministic RHS), one process
per GPU.

  python bench.py --gpus 1 --steps 200 --warmup 20                  the headline line alone
  python bench.py --gpus 1 --steps 200 --warmup 20 --full           ... and everything else this script measures
  python bench.py --gpus 1 --steps 200 --dump-outputs DIR           ... and what the timed solve computed, as DIR/<name>.npy
  python bench.py --gpus N ...                      (WORLD_SIZE unset: starts its N ranks itself)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one GCR iteration (1 SpMV + the fused orthogonalisation kernels).  The warm-up is a solve of W (at least 1)
iterations, then more solves until WARMUP_MIN_S of solving have passed; the timed region is ONE mgcr_gcr_solve call limited
to exactly K iterations (tol = 0 so it cannot stop early), inputs resident in HBM, bracketed by barrier + device
synchronisation, max over ranks: value = K / its seconds, ms_per_step = its milliseconds / K.  --dump-outputs DIR then
writes that solve's x (float64 [re, im] pairs; a fixed, seeded sample of its rows when it is larger than 64 MB) and
residual history (dump_outputs).
N > 1: the grid grows along i to (128 N) x 128 x 128 and is slab-partitioned, 128 planes (= the N=1
problem) per GPU — weak scaling; value = N * iterations/s (shard-iterations/s).

One JSON line on stdout (rank 0).  With --full it also carries `timing_repeated` (the same solve repeated until >= 0.25 s
have been timed: median, min, max), `phases` and `roofline` (the phase of the iteration that takes longest, hipEvent-timed
on the library's own stream inside a solve), `spmv` (stand-alone applies, cold and back to back), `cpu_baseline` (the real
reference, oracle/_ref/ref_harness, on the host's cores; the oracle port when that binary is absent — `kind` and
`binary` say which), `cpu_baseline_optimised` (OpenMP fused-pass CPU port) and `workloads`: the other
BASELINE.json configs, each measured by a child process of this script (`python bench.py --workload NAME` runs one alone;
--no-cpu-baseline / --no-extras leave those parts out of a --full line).

Process structure.  N = 1: the headline runs in this process (the library alone: torch is not imported), every other
workload in a child process (bounded time; a failure is recorded, never fatal).  N > 1: each rank is a SUPERVISOR that
never touches the GPU; it starts the measuring WORKER as a child process and, should the worker fail or hang on any
rank, all supervisors agree (gloo) to try again with a more conservative transport: peer-write kernels
-> plain RCCL -> host-staged.  `launch` in the JSON says what ran.  With WORLD_SIZE unset the N
supervisors are started by this script (the launcher), which exits non-zero if any of them does.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import tempfile
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable
EXTRA_WORKLOADS = ["poisson256_gcr", "mg256", "poisson512_gcr", "mg512", "ell_slab_spmv128", "irregular_spmv", "poisson128_gcr_general", "bcsr", "bcsr_mg", "sample", "latency64"]
MG_PARITY_NOTE = ("unpinned: the reference's MG::operator() returns uninitialised memory (src/MG.h:124-129,405-430), so no reference "
                  "output exists; the cycle is checked against the oracle's corrected cycle — bit for bit in the device's summation order, "
                  "cycle and MG-preconditioned solve (tests/test_gpu_mg.py)")
# transports a multi-GPU run falls back through (environment of the worker processes)
LADDER = [("default: peer-write kernels where their self-test passes, RCCL otherwise", {}),
          ("RCCL only", {"MGCR_PEER_ALLREDUCE": "0", "MGCR_PEER_HALO": "0"}),
          ("host-staged transport (slow; a flagged line instead of none)", {"MGCR_BENCH_TRANSPORT": "host"})]
ATTEMPT_TIMEOUT_S = [420, 240, 240]
WARMUP_MIN_S = 0.2      # seconds of solving before the timed steps, the --warmup steps included


# ------------------------------------------------------------------------------------------------
# launching
# ------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launcher_plan(n_gpus, argv, port, base_env=None):
    """Commands and environments of the N rank processes `python bench.py --gpus N` starts when it was not
    launched by torch.distributed.run (pure function: tests/test_bench_launcher.py checks it on CPU)."""
    base = dict(os.environ if base_env is None else base_env)
    plan = []
    for r in range(n_gpus):
        env = dict(base)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_gpus), LOCAL_WORLD_SIZE=str(n_gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (hipIpc mailboxes, RCCL)
        env.pop("MGCR_BENCH_ROLE", None)
        plan.append(([sys.executable, os.path.abspath(__file__)] + list(argv), env))
    return plan


def run_launcher(args, argv):
    """WORLD_SIZE unset and --gpus N > 1: start the N ranks (before anything here has touched the GPU), pass rank
    0's line through, exit non-zero if any rank failed."""
    procs = []
    for r, (cmd, env) in enumerate(launcher_plan(args.gpus, argv, free_port())):
        # every rank leads a process group of its own: the GPU-holding worker is the supervisor's CHILD, and ending a rank
        # must end that worker too (a killed supervisor would otherwise leave it running with the device)
        procs.append(subprocess.Popen(cmd, env=env, stdout=None if r == 0 else subprocess.DEVNULL, start_new_session=True))
    rc = 0
    deadline = time.time() + launcher_deadline_s()
    pending = list(procs)
    try:
        while pending and time.time() < deadline:
            for p in list(pending):
                if p.poll() is not None:
                    pending.remove(p)
                    rc = rc or p.returncode
            time.sleep(0.2)
    finally:
        for p in procs:   # the exact process groups started above (a rank that has exited may have left its worker behind)
            if p in pending:
                rc = rc or 1
            end_process_group(p)
    return 1 if rc else 0


def launcher_deadline_s():
    return float(os.environ.get("MGCR_BENCH_LAUNCHER_DEADLINE_S", sum(ATTEMPT_TIMEOUT_S) + 300))


def end_process_group(p):
    """SIGKILL the process group `p` leads (it was started with start_new_session=True) — the process and whatever it
    started — and reap p.  Harmless when everything has already exited."""
    import signal
    try:
        os.killpg(p.pid, signal.SIGKILL)
    except (ProcessLookupError, PermissionError):
        pass
    try:
        p.wait(timeout=10)
    except Exception:
        pass


def worker_command(argv, port, mode_env, base_env=None):
    env = dict(os.environ if base_env is None else base_env)
    # Under torch.distributed.run the supervisor's environment says TORCHELASTIC_USE_AGENT_STORE=True: init_process_group(env://) of a
    # process that inherits it does not open a store of its own on rank 0 but waits for the launcher agent's at MASTER_PORT — and the
    # workers rendezvous on a FRESH port, where nobody listens: they would hang until the attempt's time limit.  The workers are not the
    # agent's processes: they get none of its variables (and rendezvous over an explicit tcp:// address besides, worker_init_method).
    for k in list(env):
        if k.startswith("TORCHELASTIC_") or k in ("GROUP_RANK", "ROLE_RANK", "ROLE_NAME", "ROLE_WORLD_SIZE", "GROUP_WORLD_SIZE"):
            env.pop(k)
    env.update(mode_env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (hipIpc mailboxes, RCCL) — also when a launcher other than ours started the ranks
    env.update(MGCR_BENCH_ROLE="worker", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1")
    return [sys.executable, os.path.abspath(__file__)] + list(argv), env


def worker_init_method():
    """The workers' rendezvous: rank 0 of the workers hosts the store at the port its supervisor picked — stated explicitly, so that
    nothing inherited from a launcher's environment can redirect it."""
    return "tcp://%s:%s" % (os.environ.get("MASTER_ADDR", "127.0.0.1"), os.environ["MASTER_PORT"])


def last_json_line(text):
    for line in reversed(text.splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            try:
                return json.loads(line)
            except ValueError:
                continue
    return None


def run_supervisor(args, argv):
    """One per rank, N > 1.  Never touches the GPU: starts the worker as a child and walks the transport ladder with
    the other supervisors until a run succeeds on every rank."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    # gloo announces its connections on stdout ("[Gloo] Rank 0 is connected to ..."): keep stdout to the one JSON line
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)
    t_start = time.time()

    def attempt(label, mode_env, limit):
        """One collective attempt: every supervisor starts its worker with this environment; all succeed or none does."""
        port = torch.tensor([free_port() if rank == 0 else 0], dtype=torch.int64)
        dist.broadcast(port, src=0)
        cmd, env = worker_command(argv, int(port[0]), mode_env)
        t0 = time.time()
        # (files, not pipes: nobody reads while the supervisors poll below)
        with tempfile.TemporaryFile(mode="w+") as f_out, tempfile.TemporaryFile(mode="w+") as f_err:
            p = subprocess.Popen(cmd, env=env, stdout=f_out, stderr=f_err, text=True)
            # The supervisors poll in lockstep: as soon as ONE worker has failed (or run out of time) every supervisor ends its
            # own — a rank that died at start-up must not leave the others waiting in a rendezvous until the time limit.
            try:
                while True:
                    rc = p.poll()
                    if rc is None and time.time() - t0 > limit:
                        p.kill()
                        p.wait()
                        rc = -9
                    st = torch.tensor([1 if rc not in (None, 0) else 0, 1 if rc is not None else 0], dtype=torch.int32)
                    dist.all_reduce(st)
                    if int(st[0]) > 0:
                        if rc is None:
                            p.kill()       # the exact process started above
                            p.wait()
                            rc = -15       # ended because another rank's worker failed
                        break
                    if int(st[1]) == world:
                        break
                    time.sleep(0.25)
            finally:
                # whatever ends this loop — a collective that raises because a peer supervisor died included — the worker
                # (it holds the GPU) does not outlive it
                if p.poll() is None:
                    p.kill()
                    p.wait()
            f_out.seek(0)
            f_err.seek(0)
            out, err = f_out.read(), f_err.read()
        parsed = last_json_line(out) if rank == 0 else None
        good = rc == 0 and (rank != 0 or parsed is not None)
        flag = torch.tensor([1 if good else 0], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        bad = torch.tensor([0 if good else 1], dtype=torch.int32)
        dist.all_reduce(bad)
        rec = {"transport": label, "ok": bool(int(flag[0])), "ranks_failed": int(bad[0]), "seconds": round(time.time() - t0, 1),
               "rank0_rc": rc, "rank0_stderr_tail": "" if good else err[-600:]}
        if not good:
            sys.stderr.write("[bench rank %d] attempt '%s' failed (rc %s)\n%s\n" % (rank, label, rc, err[-2000:]))
        return bool(int(flag[0])), parsed, rec

    attempts, result, ok, used = [], None, False, None
    for (label, mode_env), limit in zip(LADDER, ATTEMPT_TIMEOUT_S):
        good, parsed, rec = attempt(label, mode_env, limit)
        attempts.append(rec)
        if good:
            ok, result, used = True, parsed, (label, mode_env)
            break
    # --full: configs[3] and configs[4] in their multi-GPU form, with the transport that carried the headline; bounded in time and
    # never fatal (skipped when the headline needed long: the one JSON line must not be lost to a time limit)
    extras = {}
    if ok and args is not None and args.full and not args.no_extras:
        for name in DIST_WORKLOADS:
            go = torch.tensor([1 if time.time() - t_start < 360 else 0], dtype=torch.int32)
            dist.broadcast(go, src=0)
            if not int(go[0]):
                extras[name] = {"skipped": "time budget of the run used up"}
                continue
            good, parsed, rec = attempt(used[0] + " / " + name, dict(used[1], MGCR_BENCH_WORKLOAD=name), DIST_EXTRA_TIMEOUT_S)
            extras[name] = parsed if good else {"failed": rec}
    if rank == 0:
        if ok:
            result["launch"] = {"ranks": world, "started_by": os.environ.get("MGCR_BENCH_STARTED_BY", "torch.distributed.run or bench.py launcher"),
                                "attempts": attempts}
            if extras:
                result["workloads"] = extras
            print(json.dumps(result), flush=True)
        else:
            sys.stderr.write("bench.py: no transport produced a result: %s\n" % json.dumps(attempts))
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


# ------------------------------------------------------------------------------------------------
# helpers shared by the workloads
# ------------------------------------------------------------------------------------------------
def spmv_algorithmic_bytes(nnz, nrow, ncol):
    """complex-fp64 values + int32 columns + int32 row pointers + x read once
    + y written once."""
    return nnz * 20 + (nrow + 1) * 4 + ncol * 16 + nrow * 16


def source_sha16():
    """Fingerprint of the kernel sources: a committed PMC traffic figure is only printed next to live timings when it
    was measured on exactly these sources (tools/pmc_traffic.py stamps it)."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(key, n, lims=None, restart=0):
    """(HBM bytes per launch of phase `key` measured by PMC, note) — null unless measured on the current sources.  With
    `lims` (the number of stored directions of every timed iteration) the per-kernel figures are weighted by the kernels
    those iterations launched, i.e. exactly the launches `achieved` is an average over."""
    prof = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        d = json.load(open(prof))
    except Exception:
        return None, "no profiles/pmc_traffic.json"
    if d.get("n") != n:
        return None, "profiles/pmc_traffic.json was measured at n = %s" % d.get("n")
    if d.get("src_sha16") != source_sha16():
        return None, ("profiles/pmc_traffic.json was measured on other kernel sources (%s, now %s): not printed next to live timings"
                      % (d.get("src_sha16"), source_sha16()))
    note = "PMC FETCH_SIZE / WRITE_SIZE passes of these sources (tools/pmc_traffic.py)"
    kern = d.get("kernel_hbm_bytes_per_launch")
    if lims and kern:
        import re

        have_step_build = any(name.startswith("step_build_kernel") for name in kern)
        have_step_build_xr = any(re.match(r"step_build_kernel<\d+, \d+, \d+, true, ", name) for name in kern)
        have_step_build_close = any(re.match(r"step_build_kernel<.*, true>", name) for name in kern)

        def of(l):
            for name, b in kern.items():
                if key == "xr" and name.startswith("xr_update_kernel"):
                    return b
                m = re.match(r"step_build_kernel<\d+, \d+, (\d+), (true|false), (true|false)>", name)
                if (key == "apply_dots" and m and int(m.group(1)) == l and (l < restart or m.group(3) == "true") and have_step_build and
                        (m.group(2) == "true") == have_step_build_xr):
                    return b   # (with the next step's update fused in, the few launches without it — before the solve's last step — are booked like the others)
                m = re.match(r"step_apply_kernel<\d+, \d+, (\d+)>", name)
                if key == "apply_dots" and m and int(m.group(1)) == l and not ((l < restart or have_step_build_close) and have_step_build):
                    return b
                m = re.match(r"build_lean_kernel<(\d+)>", name)
                if key == "build" and l < restart and m and int(m.group(1)) == l:
                    return b
                m = re.match(r"build_close_kernel<(\d+)", name)
                if key == "build" and l == restart and m and int(m.group(1)) == l:
                    return b
            return None
        per = [of(l) for l in lims]
        if key != "xr" and per:
            per[-1] = 0.0   # the solve's last iteration launches neither an apply nor a build (gcr_phase_model)
        if all(v is not None for v in per):
            return sum(per) / len(per), note + ", per kernel, weighted by the kernels the timed iterations launched"
    return d["phase_hbm_bytes_per_launch"].get(key), note + ", average over the launches of the profiled run"


def pmc_traffic_workload(name):
    """(HBM bytes per apply of workload `name` measured by PMC, note): profiles/pmc_traffic.json "workloads" section, only
    when it was measured on the current kernel sources."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    except Exception:
        return None, "no profiles/pmc_traffic.json"
    w = (d.get("workloads") or {}).get(name)
    if not w:
        return None, "not measured for this workload"
    if w.get("src_sha16", d.get("src_sha16")) != source_sha16():
        return None, "measured on other kernel sources (%s, now %s)" % (w.get("src_sha16", d.get("src_sha16")), source_sha16())
    return w.get("hbm_bytes_per_apply"), w.get("note", "PMC FETCH_SIZE / WRITE_SIZE passes (tools/pmc_traffic.py)")


def stats(samples):
    s = sorted(samples)
    m = len(s)
    med = s[m // 2] if m % 2 else 0.5 * (s[m // 2 - 1] + s[m // 2])
    return {"median": med, "min": s[0], "max": s[-1], "repetitions": m}


def repeat_timed(fn, min_total=0.25, min_reps=5, max_reps=400):
    """fn() -> seconds of one timed region; repeated until min_total seconds have been timed."""
    out, tot = [], 0.0
    while len(out) < min_reps or (tot < min_total and len(out) < max_reps):
        dt = fn()
        out.append(dt)
        tot += dt
    return out


def usable_cores():
    ncores = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = ncores
    # The visible core count is not the usable one: a 1-GPU box exposes 256 cores and its cgroup grants 16
    # (cpu.max "1600000 100000"); more threads than that are throttled, not run.
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            usable = max(1, min(usable, int(int(quota) / int(period) + 0.5)))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                usable = max(1, min(usable, int(q / per + 0.5)))
        except Exception:
            pass
    return usable, ncores


def cpu_baseline(n, iters=10):
    """Time the reference CPU path on this box's host cores (bounded sample: `iters` GCR
    iterations of the same system, 1 thread — the reference's Sparse/Field path is single
    threaded, src/Operator.h:330-346, src/Fields.h:192-308)."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
    ncores = os.cpu_count() or 1
    if os.path.exists(exe):
        out = subprocess.run([exe, "/tmp", "bench", str(n), str(iters)], capture_output=True, text=True, timeout=900)
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                return {"value": d["it_per_s"], "unit": "it/s", "cores": 1, "kind": "reference", "binary": "oracle/_ref/ref_harness",
                        "sample": "%d GCR iterations (restart 5) of the same Poisson %d^3 system by the real reference "
                                  "(oracle/_ref/ref_harness: the reference's own headers compiled by oracle/Makefile, g++ -O3), 1 thread of %d "
                                  "host cores" % (iters, n, ncores),
                        "spmv_seconds": d["spmv_seconds"], "host_cores": ncores}
    # oracle/_ref is git-ignored (built by __graft_entry__.build() where /root/reference exists): without it the oracle
    # port is timed instead (same operation order, fewer temporaries => faster than the reference) and says so
    from oracle import oracle as orc
    N, rowptr, col, val = orc.poisson3d(n)
    A = orc.csr(N, N, rowptr, col, val)
    b = orc.fill_rhs(N, 0)
    t0 = time.perf_counter()
    orc.gcr_solve(A, orc.gcr_param(restart=5, max_iter=iters, tol=0.0), b)
    dt = time.perf_counter() - t0
    return {"value": iters / dt, "unit": "it/s", "cores": 1, "kind": "port", "binary": "oracle/libmgcr_oracle.so (oracle/_ref/ref_harness absent)",
            "sample": "%d GCR iterations (restart 5) of the same Poisson %d^3 system by oracle/mgcr_oracle.c, 1 thread"
                      % (iters, n), "host_cores": ncores}


def cpu_baseline_optimised(n, restart, seconds=8.0):
    """SURVEY.md §8(d) "optimised CPU" row: the OpenMP port with fused passes (oracle/mgcr_cpu_opt.c) on all
    of this box's host cores, bounded to about `seconds` of work."""
    from oracle import oracle as orc
    usable, ncores = usable_cores()
    dt, _ = orc.opt_gcr_poisson(n, restart, 5, usable)          # page-in + a first rate estimate
    iters = int(max(10, min(500, seconds / max(dt / 5, 1e-6))))
    dt, hist = orc.opt_gcr_poisson(n, restart, iters, usable)
    return {"value": iters / dt, "unit": "it/s", "cores": usable, "kind": "port", "binary": "oracle/libmgcr_oracle.so",
            "sample": "%d GCR iterations (restart %d) of the same Poisson %d^3 system by oracle/mgcr_cpu_opt.c: OpenMP over "
                      "%d threads (= the CPU share this process is granted), CSR with int32 columns and real values, update / "
                      "SpMV+dots / build fused as on the GPU" % (iters, restart, n, usable),
            "final_rel_residual": float(hist[-1]), "host_cores": ncores}


def storage_name(fmt, npat):
    return {0: "ELL slab",
            1: "row-pattern dictionary, %s patterns (2 B per row + table)" % npat,
            2: "row-pattern dictionary for the columns (%s patterns) + value slab" % npat,
            3: "stencil view: %s slots, one value per slot, one 64-bit presence word per wave of 64 rows and slot" % npat}[fmt]


def gcr_phase_model(n_it, R, V, matrix_bytes, ncol, N, fused):
    """Bytes each phase of the timed iterations has to move per launch with the layout actually stored ("if
    the implementation stores something else ... it must report with its stored sizes"):
      xr      r, Ap read + r written                                              3 V
      apply   matrix + r read + Ar written + lim Aps_j read (+ Ar re-read by the separate multidot kernel when the
              fused kernel is not used)
      build   in-cycle (3 + lim) V, lim = 1..R-1;  cycle-closing step (2R + 6) V
    fused >= 2 (csrc/gcr_stepbuild.hip): the in-cycle steps run apply, dots and build as ONE launch in which A r never
    leaves the chip — matrix + r + 2 lim Aps_j + r again + Ap written = matrix + 16 ncol + (2 lim + 2) V, booked under
    `apply`; only the step that closes a cycle still has a build launch.  fused >= 3: that launch also ends with the NEXT
    iteration's residual update (+ 2 V: r read, r' written; the new Ap is on the chip), whose xr launch then does not exist.
    fused == 4: the step that closes a cycle runs the same way (restart <= 5): matrix + 16 ncol + (3 R + 5) V.  The solve's
    last iteration (the timed solves run to max_iter) has no apply and no build launch at all (finish_step_kernel): it counts
    with its residual update only — rounds 1 and 2 booked an apply and a build for it that never ran (4-8 % too many bytes in the
    whole-iteration figure at --steps 20, 5 % in the dominant phase's).
    fused == 5 (csrc/gcr_fused_xr_tile.h, the windowed regime; step_apply_xr_kernel in the latency regime): the residual update runs
    inside the apply + dots kernel — r and Ap read, r' and A r' written, the other lim - 1 direction streams read (Ap IS the newest of
    them): matrix + (3 + lim) V booked under `apply`, no xr launch; the build stays a launch of its own.  The solve's last iteration
    still updates with xr_update_kernel (3 V).
    exact for the iterations that were timed: iteration k of a cycle orthogonalises against lim = k stored directions."""
    lims = [((k - 1) % R) + 1 for k in range(1, max(n_it, 1) + 1)]
    xr_in_apply = fused == 5
    if xr_in_apply:
        fused = 1
    one = fused >= 2
    nl = len(lims)

    def one_launch(idx):            # iteration idx (0-based) runs apply + dots + build as one launch (fused == 4: the closing step too)
        return one and lims[idx] <= 5 and (lims[idx] < R or fused == 4) and idx < nl - 1

    def update_prefetched(idx):     # ... and its residual update already ran at the end of the previous iteration's launch (fused >= 3)
        return fused >= 3 and idx >= 1 and one_launch(idx - 1)

    def apply_bytes(idx):
        l = lims[idx]
        if idx == nl - 1:
            return 0      # the solve's last iteration updates x and r and records |r|; the direction it would go on to build is never used
        if one_launch(idx):
            nxt = 2 * V if (idx + 1 < nl and update_prefetched(idx + 1)) else 0    # r read again, r' written; the new Ap is on the chip
            if l == R:   # closing step in one launch: apply (without the write of A r) + build_close (without its read)
                return matrix_bytes + 16 * ncol + (3 * R + 5) * V + nxt
            return matrix_bytes + 16 * ncol + (2 * l + 2) * V + nxt
        if xr_in_apply:
            return matrix_bytes + (3 + l) * V
        return matrix_bytes + 16 * ncol + 16 * N + l * V + (0 if fused else V) + (V if l > 8 else 0)

    def build_bytes(idx):
        l = lims[idx]
        if one_launch(idx) or idx == nl - 1:
            return 0
        return (2 * R + 6) * V if l == R else (3 + l) * V
    b_xr = [0 if update_prefetched(i) or (xr_in_apply and i < nl - 1) else 3.0 * V for i in range(nl)]
    b_apply = [apply_bytes(i) for i in range(nl)]
    b_build = [build_bytes(i) for i in range(nl)]
    return [sum(b_xr) / nl, sum(b_apply) / nl, sum(b_build) / nl], sum(lims) / float(nl)


def cold_apply_ms(mg, A, xin, yout, reps, Field):
    """The stand-alone operator apply with COLD caches: between two applies a 512 MiB copy sweeps L2 and the 256 MiB
    Infinity Cache; the apply alone sits between the library's stream events."""
    import ctypes
    nf = 16 * 1024 * 1024                      # 2 x 256 MiB of complex fp64
    fa, fb = Field((nf,)).set_zero(), Field((nf,))
    t_c = ctypes.c_double()
    ts = []
    for _ in range(reps):
        fb.assign(fa)
        mg.lib().mgcr_timer_start()
        A(xin, out=yout)
        mg.lib().mgcr_timer_stop(ctypes.byref(t_c))
        ts.append(t_c.value)
    # the same sweep + events around a plain copy of one vector: what "cold" costs a kernel that does nothing else
    cp = []
    for _ in range(reps):
        fb.assign(fa)
        mg.lib().mgcr_timer_start()
        yout.assign(xin)
        mg.lib().mgcr_timer_stop(ctypes.byref(t_c))
        cp.append(t_c.value)
    del fa, fb
    return stats(ts), stats(cp)


def cold_apply_read_sweep(mg, A, xin, yout, reps, Field, nbytes):
    """The same cold measurement with a READ-ONLY sweep (a dot product over 2 x 256 MiB): the copy sweep above leaves 256 MiB of
    dirty lines in L2 / Infinity Cache whose write-back the timed kernel then competes with (~10 %); after this one the caches
    hold clean lines of other data.  Both are reported; frac_hbm_peak keeps the copy sweep (comparable with round 1)."""
    import ctypes
    nf = 16 * 1024 * 1024
    fa, fb = Field((nf,)).set_zero(), Field((nf,)).set_zero()
    t_c = ctypes.c_double()
    ts, cp = [], []
    for _ in range(reps):
        fa.dot(fb)
        mg.lib().mgcr_timer_start()
        A(xin, out=yout)
        mg.lib().mgcr_timer_stop(ctypes.byref(t_c))
        ts.append(t_c.value)
    for _ in range(reps):
        fa.dot(fb)
        mg.lib().mgcr_timer_start()
        yout.assign(xin)
        mg.lib().mgcr_timer_stop(ctypes.byref(t_c))
        cp.append(t_c.value)
    del fa, fb
    a, c = stats(ts), stats(cp)
    vb = 32 * yout.field_size()
    return {"sweep": "read-only (dot product over 2 x 256 MiB)", "ms_cold_caches": a["median"], "stats": a,
            "GBps": nbytes / a["median"] / 1e6, "frac_hbm_peak": nbytes / a["median"] / 1e6 / HBM_PEAK_GBS,
            "copy_of_one_vector_ms": c["median"], "copy_frac_hbm_peak": vb / c["median"] / 1e6 / HBM_PEAK_GBS}


# ------------------------------------------------------------------------------------------------
# the headline workload (also the N > 1 worker)
# ------------------------------------------------------------------------------------------------
def run_headline(args, with_cpu=True):
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import ctypes
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, Sparse, problems

    # one GPU: the library is the whole path (its own HIP stream; mg.init raises without a GPU, there is no CPU fallback).
    # torch only carries the control plane of a multi-GPU run.
    torch = None
    if world > 1:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
    # bring-up switches: MGCR_BENCH_ONE_GPU=1 puts every rank on GPU 0 so that the N > 1 code path can be rehearsed on a
    # one-GPU box (RCCL refuses two ranks on one device: the run then uses the host-staged transport); numbers obtained
    # that way are not benchmark results.  MGCR_BENCH_TRANSPORT=host: host-staged (gloo) transport on purpose.
    one_gpu = os.environ.get("MGCR_BENCH_ONE_GPU", "0") == "1"
    host_transport = os.environ.get("MGCR_BENCH_TRANSPORT", "rccl") == "host" or (one_gpu and world > 1)
    if one_gpu:
        local_rank = 0
    if torch is not None:
        torch.cuda.set_device(local_rank)
    mg.init(local_rank)
    dist = None
    n = args.n
    comm = None
    rccl_note = None
    if world > 1:
        # control plane (barriers, id broadcast, max-reduce of the timing) over gloo; the data path
        # (halo exchange + dot-product all-reduces) is inside libmgcr_hip.so
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=worker_init_method(), rank=rank, world_size=world)
        from mgpreconditionedgcr_amd import Comm, DistSparse
        if host_transport:
            comm = Comm.host(dist)
        else:
            try:
                comm, err = Comm.rccl(dist), None
            except Exception as e:  # noqa: BLE001
                comm, err = None, repr(e)
            bad = torch.tensor([0 if err is None else 1], dtype=torch.int32)
            dist.all_reduce(bad)
            if int(bad[0]):   # every rank leaves: the supervisors move on to the next transport
                raise SystemExit("RCCL communicator creation failed on %d rank(s): %s" % (int(bad[0]), err))
        # weak scaling: the grid grows along i, every GPU owns n planes (= the N=1 problem)
        N, ncol, rowptr, col, val = problems.poisson3d_csr(n, rank * n, (rank + 1) * n, ni=world * n)
        nnz = int(rowptr[-1])
        A = DistSparse(comm, ncol, rank * N, rowptr, col, val)
        ncol = N  # per-shard accounting below
    else:
        N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
        nnz = int(rowptr[-1])
        A = Sparse(N, ncol, rowptr, col, val)
    del rowptr, col, val
    dims = (n, n, n)
    rhs = Field(dims).fill_rhs(0, global_offset=rank * N)
    x = Field(dims)

    def barrier():
        if dist is not None:
            dist.barrier()

    def synchronize():
        mg.lib().mgcr_synchronize()
        if torch is not None:
            torch.cuda.synchronize()

    # one solver object for all runs: its work vectors are allocated by the warm-up solve and re-used
    # (GCR_Param is re-read at every solve, like the reference's GCR does with its GCR_Param*)
    gparam = GCR_Param(0, args.restart, 1, 0.0, False)
    gcr = GCR(A, gparam)

    def run(iters, profile=False):
        x.set_zero()
        gparam.max_iter, gparam.check_every, gparam.profile_spmv = iters, max(iters, 1), profile
        synchronize()
        barrier()
        t0 = time.perf_counter()
        gcr.solve(rhs, x)
        synchronize()
        dt = time.perf_counter() - t0
        barrier()
        if dist is not None:  # max over ranks
            t = torch.tensor([dt], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t[0])
        assert gcr.last_iterations == iters, (gcr.last_iterations, iters)
        return dt

    dt_w = run(max(args.warmup, 1))  # the warm-up steps: at least one untimed solve, it allocates the solver's work vectors
    # The first solves after start-up run 1-3 % slower than the ones after them (clocks, caches): keep warming up with solves of
    # about 20 ms (at most the timed length) until WARMUP_MIN_S of solving have passed.  The solve times are maxima over the ranks,
    # so every rank runs the same number of them.
    it_w, warm_s = max(args.warmup, 1), dt_w
    while warm_s < WARMUP_MIN_S:
        it_w = int(min(args.steps, max(args.restart, it_w * 0.02 / max(dt_w, 1e-6))))
        dt_w = run(it_w)
        warm_s += dt_w
    # The solver keeps a residual-history buffer of max_iter + 1 entries (and fewer direction slots for a solve shorter
    # than a restart cycle): size it for the timed solve now, with a solve that stops after its first iteration
    # (|r|/|b| <= 2 always holds), so that no allocation falls into the timed region.
    gparam.max_iter, gparam.check_every, gparam.tol = args.steps, 1, 2.0
    x.set_zero()
    gcr.solve(rhs, x)
    gparam.tol = 0.0
    # THE timed steps: one solve of exactly --steps iterations (tol = 0, it cannot stop early)
    dt = run(args.steps)
    hist = gcr.last_history
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, x.to_numpy(), hist)
    ms_per_step = dt * 1e3 / args.steps
    it_per_s = args.steps / dt
    stored = A.stored_bytes()
    fmt, npat = A.storage_format()

    out = {
        "metric": "gcr_iterations_per_sec", "value": it_per_s * world, "unit": "it/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "value_definition": "iterations/s of ONE solve on one GPU" if world == 1 else
                            "iterations/s of the ONE distributed solve (%.1f) x n_gpus: every iteration sweeps n_gpus shards of "
                            "%d^3 rows, the weak-scaling aggregate (shard-iterations per second)" % (it_per_s, n),
        "timing": {"what": "wall seconds of one solve of exactly %d iterations (barrier + synchronise on both sides, max over ranks); "
                           "value and ms_per_step come from it" % args.steps,
                   "seconds": dt},
        "per_shard_it_per_s": it_per_s,
        "one_launch_fallbacks": mg.stat("one_launch_fallbacks"),
        "config": {"workload": "3D 7-point Poisson %d^3 per GPU, unpreconditioned GCR restart %d, complex fp64, x0=0, "
                               "RHS splitmix64 seed 0" % (n, args.restart),
                   "rows": N, "nnz": nnz, "complex": True,
                   "matrix_storage": storage_name(fmt, npat),
                   "stored_matrix_bytes": stored["matrix_bytes"], "ell_width": stored["ell_width"], "tail_nnz": stored["tail_nnz"],
                   "partition": "1 GPU" if world == 1 else "slab x%d (grid %dx%dx%d), %s" % (
                       world, world * n, n, n, ("host-staged transport%s (not a result)" % (", all ranks on GPU 0" if one_gpu else ""))
                       if host_transport else "RCCL communicator; halo: %s, all-reduce: %s" % (A.halo_kind, comm.allreduce_kind))},
        "final_rel_residual": float(hist[-1]),
        "kernel_sources_sha16": source_sha16(),
    }
    if args.full:
        # everything the line carries besides the timed steps: the same solve repeated (median), per-phase in-situ timings,
        # stand-alone SpMV figures, the roofline of the dominant phase, the N > 1 scaling baseline and collective costs, the
        # CPU baselines.  The repetitions run until >= 0.25 s have been timed; their number must be the same on every rank:
        # rank 0 decides from the timed solve
        reps = int(min(400, max(5, 0.25 / max(dt, 1e-6))))
        if dist is not None:
            t = torch.tensor([reps], dtype=torch.int64)
            dist.broadcast(t, src=0)
            reps = int(t[0])
        st = stats([dt] + [run(args.steps) for _ in range(reps - 1)])

        # Per-phase timing IN SITU: one more solve of the same length with hipEvents (library stream) between
        # the phases of every iteration — back-to-back replays of one kernel would be served from the
        # 256 MiB Infinity Cache once its operands fit, which at this size they do.
        run(args.steps, profile=True)
        ph_ms = (ctypes.c_double * 3)()
        n_it, fused = ctypes.c_int32(), ctypes.c_int32()
        mg.lib().mgcr_gcr_last_profile(ph_ms, ctypes.byref(n_it), ctypes.byref(fused))
        ph_us = [1e3 * v / max(n_it.value, 1) for v in ph_ms]           # average microseconds per iteration
        y = Field(dims)
        spmv_ms_replay = A.bench_apply(rhs, y, reps=args.spmv_reps)
        cold, cold_copy = (None, None)
        if world == 1:
            cold, cold_copy = cold_apply_ms(mg, A, rhs, y, args.spmv_reps, Field)
        cold_read = cold_apply_read_sweep(mg, A, rhs, y, args.spmv_reps, Field, stored["matrix_bytes"] + 16 * ncol + 16 * N) if world == 1 else None
        V = 16 * N
        R = args.restart
        b_phase, mean_lim = gcr_phase_model(n_it.value, R, V, stored["matrix_bytes"], ncol, N, fused.value)
        names = ["xr_update_kernel (alpha, residual ring, |r|^2)" if fused.value != 5 else "(no launch but the solve's last update: the residual update runs inside the apply kernel)",
                 "step_apply_kernel (SpMV + beta dot products, one kernel)" if fused.value == 1 else
                 "step_apply_xr*_kernel (residual update + SpMV + beta dot products, one kernel)" if fused.value == 5 else "SpMV + multidot_kernel",
                 "build_lean_kernel<1..%d> / build_close_kernel<%d> (direction build + x update)" % (R - 1, R)]
        if fused.value >= 2:
            names[0] = "xr_update_kernel (alpha, residual ring, |r|^2)" + (
                ": only the updates that open or end the solve%s — the others run at the end of step_build_kernel" % ("" if fused.value == 4 else " or follow a cycle's closing step") if fused.value >= 3 else "")
            names[1] = ("step_build_kernel<1..%d> (SpMV + beta dot products + direction build%s in ONE launch, A r stays in LDS)%s"
                        % (R if fused.value == 4 else R - 1, " + the next step's residual update" if fused.value >= 3 else "",
                           "" if fused.value == 4 else "; the step that closes a cycle: step_apply_kernel<%d>" % R))
            names[2] = ("(no launch: every step builds inside step_build_kernel; what is timed here are the event records of an empty slot)" if fused.value == 4 else
                        "build_close_kernel<%d> (the step that closes a cycle; the other steps build inside step_build_kernel)" % R)
        keys = ["xr", "apply_dots", "build"]
        dom = max(range(3), key=lambda k: ph_us[k])
        achieved = b_phase[dom] / (ph_us[dom] * 1e-6) / 1e9
        lims_timed = [((k - 1) % R) + 1 for k in range(1, max(n_it.value, 1) + 1)]
        traffic, traffic_note = pmc_traffic(keys[dom], n, lims_timed, R) if world == 1 else (None, "N > 1")
        b_spmv_survey = spmv_algorithmic_bytes(nnz, N, ncol)
        iter_bytes_survey = b_spmv_survey + (13 + 3 * mean_lim) * V   # SURVEY.md §8(d) accounting
        iter_bytes_ours = sum(b_phase)                                # what this implementation moves
        spmv_bytes = stored["matrix_bytes"] + 16 * ncol + 16 * N
        cold_ms = cold["median"] if cold else None

        # N > 1: what ONE GPU does on its own shard with the kernel path the distributed solve runs — the three kernels per
        # iteration; the one-launch steps (gcr_stepbuild.hip) stop at the process boundary, their in-launch sums do not cross GPUs —
        # so that per_shard_it_per_s / scaling_baseline_it_per_s is the price of the communication alone, and the N = 1 headline
        # (one-launch steps) is not what an N-GPU line gets divided by.  Every rank measures its own shard; the slowest counts.
        scaling_baseline = None
        if world > 1:
            Nl, ncl, rp, ci, va = problems.poisson3d_csr(n)
            Aloc = Sparse(Nl, ncl, rp, ci, va)
            del rp, ci, va
            prev_sb, prev_res = mg.set_option("step_build", 0), mg.set_option("resident_solver", 0)
            try:
                gl = GCR(Aloc, GCR_Param(0, args.restart, args.steps, 0.0, False, check_every=args.steps))
                xl, rl = Field(dims), Field(dims).fill_rhs(0)
                timed_solve(mg, gl, rl, xl)
                sb = stats(repeat_timed(lambda: timed_solve(mg, gl, rl, xl), min_total=0.15, min_reps=5))
            finally:
                mg.set_option("step_build", prev_sb)
                mg.set_option("resident_solver", prev_res)
            t = torch.tensor([sb["median"]], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            scaling_baseline = {"it_per_s": args.steps / float(t[0]), "this_rank_seconds": sb,
                                "what": "single-GPU solve of one %d^3 shard, same %d iterations, three kernels per iteration (step_build and the resident "
                                        "solver off: the path a distributed shard runs); max over ranks" % (n, args.steps)}
            del Aloc, gl, xl, rl

        out.update({
            "timing_repeated": {"what": "the timed solve repeated until >= 0.25 s have been timed (the first repetition is the timed solve itself)",
                                "seconds": st, "it_per_s_median": args.steps / st["median"] * world,
                                "it_per_s_min": args.steps / st["max"] * world, "it_per_s_max": args.steps / st["min"] * world},
            "scaling_baseline_it_per_s": None if scaling_baseline is None else scaling_baseline["it_per_s"],
            "scaling_baseline": scaling_baseline,
            "phases": {keys[k]: {"kernel": names[k], "us_per_iteration": ph_us[k], "bytes_per_launch": b_phase[k],
                                 "GBps": b_phase[k] / (ph_us[k] * 1e-6) / 1e9 if ph_us[k] > 0 else None} for k in range(3)},
            "phases_timed": "in situ: hipEvents between the phases of each of the %d iterations of a GCR solve" % n_it.value,
            "spmv": {"kernel": "stand-alone operator apply (inside the solver loop it runs fused with the beta dot products: phases.apply_dots)",
                     "ms_cold_caches": cold_ms, "ms_cold_caches_stats": cold, "ms_back_to_back_replay": spmv_ms_replay,
                     "includes_halo_exchange": world > 1,
                     "bytes_moved_stored_layout": spmv_bytes,
                     "GBps": None if not cold_ms else spmv_bytes / cold_ms / 1e6,
                     "frac_hbm_peak": None if not cold_ms else spmv_bytes / cold_ms / 1e6 / HBM_PEAK_GBS,
                     "GBps_back_to_back": spmv_bytes / spmv_ms_replay / 1e6,
                     "copy_of_one_vector_same_conditions": None if not cold_copy else {
                         "ms_cold_caches": cold_copy["median"], "bytes": 2 * V, "GBps": 2 * V / cold_copy["median"] / 1e6,
                         "frac_hbm_peak": 2 * V / cold_copy["median"] / 1e6 / HBM_PEAK_GBS,
                         "note": "a plain y = x between the same cache sweep and the same stream events: the ceiling a cold "
                                 "%d-row kernel has under this measurement" % N},
                     "cold_caches_read_only_sweep": cold_read,
                     "algorithmic_bytes_survey_formula": b_spmv_survey,
                     "GBps_survey_formula": None if not cold_ms else b_spmv_survey / cold_ms / 1e6},
            "iteration": {"bytes_moved_model": iter_bytes_ours, "GBps": iter_bytes_ours / (ms_per_step * 1e-3) / 1e9,
                          "frac_hbm_peak": iter_bytes_ours / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "algorithmic_bytes_survey": iter_bytes_survey,
                          "GBps_survey": iter_bytes_survey / (ms_per_step * 1e-3) / 1e9},
            "roofline": {"kernel": names[dom], "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_note": traffic_note, "bytes_per_launch": b_phase[dom],
                         "us_per_launch": ph_us[dom],
                         "note": "dominant phase of the iteration by time; achieved = bytes of the stored layout the phase's "
                                 "kernel has to move per launch (average over a restart cycle) / its hipEvent-timed duration"
                                 + ("" if world == 1 else "; N > 1: the phase times include the halo exchange (apply_dots) and both "
                                                          "all-reduces of the iteration (build)")},
        })
        if world > 1:
            # what the iteration's two all-reduces (4 doubles; 1 + 2 lim doubles) and its halo exchange cost on their own
            us = ctypes.c_double()
            comm_us = {}
            for cnt in (4, 1 + 2 * args.restart):
                mg.lib().mgcr_comm_bench_allreduce(comm.h, cnt, 50, ctypes.byref(us))
                comm_us["allreduce_%d_doubles_us" % cnt] = us.value
            out["comm"] = comm_us
            out["comm"]["allreduce_kind"] = comm.allreduce_kind
            out["comm"]["halo_kind"] = A.halo_kind
            out["comm"]["ranks"] = comm.size
            out["comm"]["transport"] = "host-staged" if host_transport else "RCCL"
            out["comm"]["spmv_with_halo_exchange_ms_replay"] = spmv_ms_replay
        if rank == 0 and world == 1 and with_cpu:
            try:
                out["cpu_baseline"] = cpu_baseline(n)
            except Exception as e:  # the baseline leg must never take the GPU numbers down with it
                out["cpu_baseline"] = {"value": None, "unit": "it/s", "cores": 1, "kind": "reference", "sample": "failed: %r" % (e,)}
            try:
                out["cpu_baseline_optimised"] = cpu_baseline_optimised(n, args.restart)
            except Exception as e:
                out["cpu_baseline_optimised"] = {"value": None, "unit": "it/s", "cores": None, "kind": "port", "sample": "failed: %r" % (e,)}
        del y
    # orderly teardown: solver state and operator first, then the communicator, then the process group
    del gcr, x, rhs
    del A
    if dist is not None:
        dist.barrier()
        lib = mg.lib()
        lib.mgcr_synchronize()
        lib.mgcr_comm_destroy(comm.h)
        comm.h = None
        dist.destroy_process_group()
    mg.finalize()
    return out


DUMP_LIMIT_BYTES = 64 * 1000 * 1000


def dump_outputs(dirname, x, hist):
    """--dump-outputs DIR: what the timed solve returned to its caller — the solution x (complex, stored as float64 pairs
    [re, im]) and the residual history |r_k| / |b| — as DIR/<name>.npy.  An x larger than the room the history leaves under
    DUMP_LIMIT_BYTES is written as a fixed, seeded sample of its rows (x_sample.npy, rows in ascending order)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    xr = np.ascontiguousarray(x).view(np.float64).reshape(-1, 2)
    room = (DUMP_LIMIT_BYTES - hist.nbytes - 4096) // 16
    name = "x"
    if xr.shape[0] > room:
        idx = np.sort(np.random.default_rng(0).choice(xr.shape[0], size=room, replace=False))
        xr, name = xr[idx], "x_sample"
    np.save(os.path.join(dirname, name + ".npy"), xr)
    np.save(os.path.join(dirname, "residual_history.npy"), hist)


# ------------------------------------------------------------------------------------------------
# the other BASELINE.json configs (single GPU; each runs in its own process: python bench.py --workload NAME)
# ------------------------------------------------------------------------------------------------
def timed_solve(mg, gcr, rhs, x, x0=None):
    if x0 is None:
        x.set_zero()
    else:
        x.assign(x0)
    mg.lib().mgcr_synchronize()
    t0 = time.perf_counter()
    gcr.solve(rhs, x)
    mg.lib().mgcr_synchronize()
    return time.perf_counter() - t0


def wl_poisson256_gcr(args):
    """configs[1]'s solver at 256^3 — the working set (12 vectors of 268 MB) is far beyond the 256 MiB Infinity Cache, so
    this is the honest HBM point of the GCR iteration."""
    return poisson_gcr_workload(256, 50, "3D 7-point Poisson 256^3, unpreconditioned GCR restart 5, complex fp64 (configs[1]'s solver at configs[2]'s size)")


def wl_poisson512_gcr(args):
    """configs[3]'s grid — 512^3, 134 M rows, 2.1 GB per vector — on ONE MI355X (the reference partitions it over 8 devices; 288 GB of HBM
    hold the solver's ~14 vectors several times over): the plane-walk row map's largest plane (256 workgroups per band, 2 bands)."""
    return poisson_gcr_workload(512, 25, "3D 7-point Poisson 512^3 (configs[3]'s grid) on ONE GPU, unpreconditioned GCR restart 5, complex fp64")


def poisson_gcr_workload(n, iters, title):
    import ctypes
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, Sparse, problems
    mg.init(0)
    R = 5
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    nnz = int(rowptr[-1])
    A = Sparse(N, ncol, rowptr, col, val)
    del rowptr, col, val
    dims = (n, n, n)
    rhs, x, y = Field(dims).fill_rhs(0), Field(dims), Field(dims)
    prm = GCR_Param(0, R, iters, 0.0, False, check_every=iters)
    gcr = GCR(A, prm)
    timed_solve(mg, gcr, rhs, x)
    st = stats(repeat_timed(lambda: timed_solve(mg, gcr, rhs, x), min_total=0.25, min_reps=5))
    prm.profile_spmv = True
    timed_solve(mg, gcr, rhs, x)
    ph, na, fu = (ctypes.c_double * 3)(), ctypes.c_int32(), ctypes.c_int32()
    mg.lib().mgcr_gcr_last_profile(ph, ctypes.byref(na), ctypes.byref(fu))
    ph_us = [1e3 * v / max(na.value, 1) for v in ph]
    stored = A.stored_bytes()
    fmt, npat = A.storage_format()
    V = 16 * N
    b_phase, mean_lim = gcr_phase_model(na.value, R, V, stored["matrix_bytes"], ncol, N, fu.value)
    keys = ["xr", "apply_dots", "build"]
    dom = max(range(3), key=lambda k: ph_us[k])
    ms = st["median"] * 1e3 / iters
    cold, cold_copy = cold_apply_ms(mg, A, rhs, y, 10, Field)
    spmv_bytes = stored["matrix_bytes"] + 2 * V
    cold_read = cold_apply_read_sweep(mg, A, rhs, y, 10, Field, spmv_bytes)
    b_survey = spmv_algorithmic_bytes(nnz, N, ncol) + (13 + 3 * mean_lim) * V
    return {"workload": title,
            "rows": N, "nnz": nnz, "residual_update": "inside the windowed apply kernel (phases.xr: no launch)" if fu.value == 5 else "xr_update_kernel", "matrix_storage": storage_name(fmt, npat), "iterations_per_solve": iters,
            "it_per_s": iters / st["median"], "ms_per_iteration": ms, "timing_seconds": st,
            "phases": {keys[k]: {"us_per_iteration": ph_us[k], "bytes_per_launch": b_phase[k], "GBps": b_phase[k] / ph_us[k] / 1e3} for k in range(3)},
            "iteration": {"bytes_moved_model": sum(b_phase), "GBps": sum(b_phase) / ms / 1e6, "frac_hbm_peak": sum(b_phase) / ms / 1e6 / HBM_PEAK_GBS,
                          "algorithmic_bytes_survey": b_survey, "GBps_survey": b_survey / ms / 1e6},
            "roofline": {"kernel": keys[dom], "bound": "hbm", "achieved": b_phase[dom] / ph_us[dom] / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": b_phase[dom] / ph_us[dom] / 1e3 / HBM_PEAK_GBS, "traffic": None, "bytes_per_launch": b_phase[dom]},
            "spmv": {"ms_cold_caches": cold["median"], "stats": cold, "bytes_moved_stored_layout": spmv_bytes,
                     "GBps": spmv_bytes / cold["median"] / 1e6, "frac_hbm_peak": spmv_bytes / cold["median"] / 1e6 / HBM_PEAK_GBS,
                     "copy_of_one_vector_ms": cold_copy["median"], "copy_frac_hbm_peak": 2 * V / cold_copy["median"] / 1e6 / HBM_PEAK_GBS,
                     "cold_caches_read_only_sweep": cold_read}}


def wl_mg256(args):
    """configs[2]: Poisson 256^3, 3-level aggregation MG (2^3 aggregates, piecewise-constant P, Galerkin) as flexible right
    preconditioner of GCR restart 5; smoother 2 GCR sweeps, coarsest solve GCR tol 1e-2 / 50 iterations (src/main.cpp:841)."""
    return mg_poisson_workload(256, 2, "3D 7-point Poisson 256^3, 3-level MG V-cycle preconditioner (2^3 aggregates), flexible GCR restart 5 to 1e-8, fp64 (configs[2])")


def wl_mg512(args):
    """configs[3]'s problem — 512^3, MG-preconditioned GCR — on ONE MI355X: 4 levels (512^3 .. 64^3, the coarsest solve stays the
    one-launch resident solver of configs[2]); level 0 alone is 134 M rows, 2.1 GB per vector."""
    return mg_poisson_workload(512, 3, "3D 7-point Poisson 512^3 (configs[3]'s problem) on ONE GPU, 4-level MG V-cycle preconditioner (2^3 aggregates), flexible GCR restart 5 to 1e-8, fp64")


def mg_poisson_workload(n, levels, title):
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, MG, MG_Param, Mesh, Sparse, problems
    mg.init(0)
    tol = 1e-8
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    nnz = int(rowptr[-1])
    A = Sparse(N, ncol, rowptr, col, val)
    del rowptr, col, val
    dims = (n, n, n)
    rhs, x, y = Field(dims).fill_rhs(0), Field(dims).set_zero(), Field(dims)
    t0 = time.perf_counter()
    prm = MG_Param(Mesh(dims), 2, 1, None, GCR(GCR_Param(0, 10, 50, 1e-2, False)), GCR(GCR_Param(0, 10, 2, 1e-30, False)),
                   levels, None, None, null_vectors=np.ones((1, N), np.complex128))
    M = MG(A, prm)
    mg.lib().mgcr_synchronize()
    setup_s = time.perf_counter() - t0
    M(rhs, out=y)

    def cycle():
        mg.lib().mgcr_synchronize()
        t = time.perf_counter()
        M(rhs, out=y)
        mg.lib().mgcr_synchronize()
        return time.perf_counter() - t
    vc = stats(repeat_timed(cycle, min_total=0.2, min_reps=10 if n <= 256 else 5))
    # SURVEY.md §8(d) "algorithmic bytes — V-cycle": per level nu_pre + nu_post smoother iterations B_iter(lim) =
    # B_spmv + (13 + 3 lim) V with lim = 1, 2, the residual B_spmv + 2 V, restrict V_l + V_(l+1), prolong+add V_(l+1) + 2 V_l
    # What THIS implementation moves per level above the coarsest (V = one vector of the level, Vc of the next) —
    # pre-smoother: A b + dots (b read, Ap0 written: 2 V), residual update + A r1 + dots (b, Ap0 read, r1, A r1 written: 4 V; as two
    # launches where the update is not fused: 3 V + 2 V... booked at the fused count), build (A r1, r1, Ap0 read, Ap1 written: 4 V);
    # restrict from the recurrence (r1, Ap1, member list: 2.25 V + Vc); prolong + pending x (b, r1, aggregate ids read, x written:
    # 3.25 V + Vc; the prolongator is one number); post-smoother: b - A x (3 V), A r0 + dots (2 V: |b|^2 is the pre-smoother's), update +
    # A r1 + dots (4 V), build without the write of Ap1 (3 V), x += (x, r0, r1 read, x written: 4 V): 31.5 V + 2 Vc.
    tot, moved, nl = 0, 0, n
    for _ in range(levels):
        Nl, nnzl = nl ** 3, 7 * nl ** 3 - 6 * nl ** 2
        Vl, Vc = 16 * Nl, 16 * (nl // 2) ** 3
        bsp = nnzl * 20 + (Nl + 1) * 4 + 2 * Vl
        tot += 2 * sum(bsp + (13 + 3 * lim) * Vl for lim in (1, 2)) + bsp + 2 * Vl + Vl + Vc + Vc + 2 * Vl
        moved += 31.5 * Vl + 2 * Vc
        nl //= 2
    outer = GCR(A, GCR_Param(0, 5, 200, tol, False, None, M, flexible=True, check_every=2))
    timed_solve(mg, outer, rhs, x)
    sv = stats(repeat_timed(lambda: timed_solve(mg, outer, rhs, x), min_total=0.3, min_reps=3, max_reps=10 if n <= 256 else 3))
    r = rhs - A(x)
    return {"workload": title,
            "parity": MG_PARITY_NOTE, "rows": N, "nnz": nnz, "levels": [M.level_info(l) for l in range(levels + 1)],
            "mg_setup_seconds": setup_s, "vcycle_ms": vc["median"] * 1e3, "vcycle_timing_seconds": vc,
            "vcycle_bytes_survey_model_excl_coarsest": tot, "vcycle_GBps_survey": tot / vc["median"] / 1e9,
            "vcycle_bytes_moved_model_excl_coarsest": moved, "vcycle_GBps_moved_lower_bound": moved / vc["median"] / 1e9,
            "vcycle_frac_hbm_peak_moved_lower_bound": moved / vc["median"] / 1e9 / HBM_PEAK_GBS,
            "vcycle_moved_model": "31.5 V + 2 V_coarse per level above the coarsest (round 2: 44 V); the coarsest solve (one launch, latency-bound) moves next to nothing, its time is in the denominator",
            "outer_iterations": outer.last_iterations, "converged": outer.last_converged, "seconds_to_tol": sv["median"],
            "solve_timing_seconds": sv, "tol": tol, "final_rel_residual": float(outer.last_history[-1]),
            "true_rel_residual": r.norm() / rhs.norm()}


def wl_ell_slab_spmv128(args):
    """The general-matrix SpMV path (north_star's "CSR/ELL-hybrid layout with coalesced HBM row reads"): the same 128^3
    Poisson matrix with the row-pattern dictionary switched off, i.e. as any unstructured matrix is stored — ELL slab
    (real values here: every imaginary part is zero) + int32 columns."""
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, Sparse, problems
    mg.init(0)
    n = 128
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    nnz = int(rowptr[-1])
    prev = mg.set_option("pattern_storage", 0)
    try:
        A = Sparse(N, ncol, rowptr, col, val)
        Ac = Sparse(N, ncol, rowptr, col, val * (1.0 + 0.25j))   # complex values: 20 B per stored entry
    finally:
        mg.set_option("pattern_storage", prev)
    del rowptr, col, val
    out = {"workload": "SpMV alone, 3D 7-point Poisson 128^3 stored as a general matrix (pattern_storage=0): ELL slab, int32 columns",
           "rows": N, "nnz": nnz}
    xf, yf = Field((n, n, n)).fill_rhs(0), Field((n, n, n))
    for tag, op in (("real_values", A), ("complex_values", Ac)):
        stored = op.stored_bytes()
        fmt, npat = op.storage_format()
        b = stored["matrix_bytes"] + 32 * N
        cold, cold_copy = cold_apply_ms(mg, op, xf, yf, 30, Field)
        warm = op.bench_apply(xf, yf, reps=50)
        out[tag] = {"matrix_storage": storage_name(fmt, npat), "ell_width": stored["ell_width"], "bytes_moved_stored_layout": b,
                    "ms_cold_caches": cold["median"], "stats": cold, "GBps": b / cold["median"] / 1e6,
                    "frac_hbm_peak": b / cold["median"] / 1e6 / HBM_PEAK_GBS, "ms_back_to_back": warm, "GBps_back_to_back": b / warm / 1e6,
                    "algorithmic_bytes_survey_formula": spmv_algorithmic_bytes(nnz, N, ncol)}
    out["roofline"] = {"kernel": "ell_spmv_rowthread (complex slab)", "bound": "hbm", "achieved": out["complex_values"]["GBps"],
                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": out["complex_values"]["frac_hbm_peak"], "traffic": None}
    return out


def wl_bcsr(args):
    """configs[4] on one GPU: unstructured HierarchicalSparse, bs = 20, skewed blocks/row (80 % of the rows 5-9 blocks, 20 %
    10-64), ~3 GB of blocks, diagonally dominant: apply GB/s and GCR on it."""
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, HierarchicalSparse
    mg.init(0)
    bs, nb = 20, 36000
    rows, cols, blocks = make_unstructured_blocks(nb, bs)
    nblk = rows.size
    H = HierarchicalSparse(nb, nb, rows, cols, blocks)
    del blocks
    n = nb * bs
    xf, yf = Field((n,)).fill_rhs(1), Field((n,))
    H(xf, out=yf)
    ms = stats([H.bench_apply(xf, yf, reps=10) for _ in range(7)])   # 3 GB per apply: nothing survives in a cache
    b_alg = nblk * (bs * bs * 16 + 4) + (nb + 1) * 4 + 2 * n * 16
    rhs, x = Field((n,)).fill_rhs(2), Field((n,))
    gcr = GCR(H, GCR_Param(0, 5, 200, 1e-10, False, check_every=5))
    timed_solve(mg, gcr, rhs, x)
    sv = stats(repeat_timed(lambda: timed_solve(mg, gcr, rhs, x), min_total=0.2, min_reps=3, max_reps=10))
    r = rhs - H(x)
    return {"workload": "unstructured HierarchicalSparse (block-CSR, bs 20, 5-64 blocks/row), apply + GCR restart 5 to 1e-10, 1 GPU (configs[4]'s operator)",
            "block_rows": nb, "bs": bs, "blocks": int(nblk), "matrix_GB": nblk * bs * bs * 16 / 1e9, "apply_ms": ms["median"], "apply_ms_stats": ms,
            "algorithmic_bytes": b_alg, "GBps": b_alg / ms["median"] / 1e6,
            "roofline": {"kernel": "bcsr_wave_kernel_t", "bound": "hbm", "achieved": b_alg / ms["median"] / 1e6, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": b_alg / ms["median"] / 1e6 / HBM_PEAK_GBS, "traffic": None},
            "gcr_iterations": gcr.last_iterations, "gcr_converged": gcr.last_converged, "gcr_seconds": sv["median"], "gcr_timing_seconds": sv,
            "gcr_it_per_s": gcr.last_iterations / sv["median"], "true_rel_residual": r.norm() / rhs.norm()}


def wl_irregular_spmv(args):
    """Two matrices of the same skewed row-length distribution: "scattered" (columns within +-2^17 rows: every gathered entry is its
    own L2 request — the gather-bound regime, profiles/r03_gather_lab.txt) and "banded" (columns within +-900 rows, as after a
    bandwidth-reducing ordering: the slab kernel stages x in an LDS window).  MGCR_BENCH_IRREGULAR_WINDOW=<w> measures one window only."""
    if os.environ.get("MGCR_BENCH_IRREGULAR_WINDOW"):
        return irregular_spmv_one(int(os.environ["MGCR_BENCH_IRREGULAR_WINDOW"]))
    sc = irregular_spmv_one(1 << 17)
    bd = irregular_spmv_one(900)
    out = {"workload": sc["workload"], "scattered_columns": sc, "banded_columns": bd,
           "roofline": dict(sc["roofline"], note="the scattered matrix (the harder case); banded: frac %.3f" % bd["roofline"]["frac"])}
    return out


def irregular_spmv_one(window):
    """north_star's layout for GENERAL matrices measured at HBM scale: an irregular scalar CSR of ~2 GB —
    80 % of the rows 5-9 entries, 20 % 10-64, a handful of rows ~2000 — stored as ELL slab + CSR tail.  The two kernels of the
    hybrid are timed separately (mgcr_set_option("spmv_part")) and together, cold (a 512 MiB copy sweeps the caches between
    applies).  Reference apply: src/Operator.h:330-346.  Checks at full size: ELL part + tail part == the whole apply bit for
    bit, and 2000 sampled rows against a host loop in the reference's order."""
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, Sparse, problems
    mg.init(0)
    N = int(os.environ.get("MGCR_BENCH_IRREGULAR_ROWS", 8 * 1024 * 1024))
    rng = np.random.default_rng(12)
    t0 = time.perf_counter()
    rowptr, col, val = problems.skewed_csr(N, rng, window=window, long_rows=64)
    gen_s = time.perf_counter() - t0
    nnz = int(rowptr[-1])
    t0 = time.perf_counter()
    A = Sparse(N, N, rowptr, col, val)
    build_s = time.perf_counter() - t0
    lay, stored = A.ell_layout(), A.stored_bytes()
    fmt, npat = A.storage_format()
    W, tail_nnz, tail_rows = lay["ell_width"], stored["tail_nnz"], lay["tail_rows"]
    lens = np.diff(rowptr)
    ell_nnz = int(np.minimum(lens, W).sum())
    npad = (N + 63) // 64 * 64
    b_ell = npad * W * 20 + 32 * N                       # slab (values + int32 columns, padding included) + x read once + y written
    b_tail = tail_nnz * 20 + tail_rows * (8 + 4 + 32)     # entries + (row id, pointer, y read-modify-write) per tail row; x is booked with the ELL part
    xf, yf, y1 = Field((N,)).fill_rhs(0), Field((N,)), Field((N,))
    A(xf, out=yf)
    # parts: ELL kernel then tail kernel into the same y == the whole apply
    mg.set_option("spmv_part", 1); A(xf, out=y1)
    mg.set_option("spmv_part", 2); A(xf, out=y1)
    mg.set_option("spmv_part", 0)
    yh = yf.to_numpy()
    parts_equal = bool(np.array_equal(yh, y1.to_numpy()))
    xh = xf.to_numpy()
    worst = 0.0
    for r in np.concatenate([rng.integers(0, N, 1990), np.argsort(lens)[-10:]]):
        acc = 0j
        for l in range(rowptr[r], rowptr[r + 1]):
            acc += val[l] * xh[col[l]]
        worst = max(worst, abs(acc - yh[r]) / max(abs(acc), 1.0))
    out = {"workload": "SpMV alone, irregular scalar CSR (80 % of rows 5-9 entries, 20 % 10-64, 64 rows ~2000; columns within +-window of the row), "
                       "ELL slab + CSR tail, complex fp64 (north_star's general-matrix layout; configs[4] 'irregular nnz/row')",
           "rows": N, "nnz": nnz, "column_window": window, "generate_seconds": gen_s, "build_seconds": build_s, "matrix_storage": storage_name(fmt, npat),
           "ell_width": W, "lanes_per_row": lay["lanes"], "x_window_in_lds": lay["x_window"], "ell_entries": ell_nnz, "ell_padding_fraction": 1.0 - ell_nnz / float(npad * W),
           "tail_rows": tail_rows, "tail_entries": tail_nnz, "matrix_GB_stored": stored["matrix_bytes"] / 1e9,
           "check_parts_sum_to_whole_bitwise": parts_equal, "check_sampled_rows_max_rel_err": worst}
    del rowptr, col, val
    for tag, part, nbytes in (("whole", 0, b_ell + b_tail), ("ell_part", 1, b_ell), ("tail_part", 2, b_tail)):
        mg.set_option("spmv_part", part)
        try:
            cold, _ = cold_apply_ms(mg, A, xf, yf, 12, Field)
            warm = A.bench_apply(xf, yf, reps=10)
        finally:
            mg.set_option("spmv_part", 0)
        out[tag] = {"bytes_moved_stored_layout": nbytes, "ms_cold_caches": cold["median"], "stats": cold, "GBps": nbytes / cold["median"] / 1e6,
                    "frac_hbm_peak": nbytes / cold["median"] / 1e6 / HBM_PEAK_GBS, "ms_back_to_back": warm, "GBps_back_to_back": nbytes / warm / 1e6}
    out["algorithmic_bytes_survey_formula"] = spmv_algorithmic_bytes(nnz, N, N)
    out["GBps_survey_formula"] = out["algorithmic_bytes_survey_formula"] / out["whole"]["ms_cold_caches"] / 1e6
    del A, xf, yf, y1
    tr, note = pmc_traffic_workload("irregular_spmv_w%d" % window)
    out["roofline"] = {"kernel": "ell_spmv_rowthread + csr_tail_kernel (whole apply)", "bound": "hbm", "achieved": out["whole"]["GBps"], "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": out["whole"]["frac_hbm_peak"], "traffic": tr, "traffic_note": note,
                       "bytes_per_launch": b_ell + b_tail}
    return out


def wl_poisson128_gcr_general(args):
    """The headline solve on GENERAL storage: Poisson 128^3, GCR restart 5, with the row-pattern dictionary and
    the stencil view switched off — the matrix is an ELL slab with int32 columns, as any matrix without repeating rows is stored.
    it/s and whole-iteration bytes / time."""
    import ctypes
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, Sparse, problems
    mg.init(0)
    n, R, iters = 128, 5, 20
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    nnz = int(rowptr[-1])
    out = {"workload": "3D 7-point Poisson 128^3, unpreconditioned GCR restart 5, complex fp64, matrix stored as a GENERAL matrix (pattern_storage=0): "
                       "ELL slab + int32 columns", "rows": N, "nnz": nnz, "iterations_per_solve": iters}
    dims = (n, n, n)
    rhs, x = Field(dims).fill_rhs(0), Field(dims)
    prev = mg.set_option("pattern_storage", 0)
    try:
        ops = {"real_values_12B_per_entry": Sparse(N, ncol, rowptr, col, val), "complex_values_20B_per_entry": Sparse(N, ncol, rowptr, col, val * (1.0 + 0.25j))}
    finally:
        mg.set_option("pattern_storage", prev)
    del rowptr, col, val
    V = 16 * N
    for tag, A in ops.items():
        prm = GCR_Param(0, R, iters, 0.0, False, check_every=iters)
        gcr = GCR(A, prm)
        timed_solve(mg, gcr, rhs, x)
        st = stats(repeat_timed(lambda: timed_solve(mg, gcr, rhs, x), min_total=0.25, min_reps=5))
        prm.profile_spmv = True
        gcr = GCR(A, prm)
        timed_solve(mg, gcr, rhs, x)
        ph, na, fu = (ctypes.c_double * 3)(), ctypes.c_int32(), ctypes.c_int32()
        mg.lib().mgcr_gcr_last_profile(ph, ctypes.byref(na), ctypes.byref(fu))
        ph_us = [1e3 * v / max(na.value, 1) for v in ph]
        stored = A.stored_bytes()
        fmt, npat = A.storage_format()
        b_phase, mean_lim = gcr_phase_model(na.value, R, V, stored["matrix_bytes"], ncol, N, fu.value)
        ms = st["median"] * 1e3 / iters
        keys = ["xr", "apply_dots", "build"]
        out[tag] = {"matrix_storage": storage_name(fmt, npat), "matrix_bytes": stored["matrix_bytes"], "it_per_s": iters / st["median"], "ms_per_iteration": ms,
                    "timing_seconds": st, "fused_apply": fu.value,
                    "phases": {keys[k]: {"us_per_iteration": ph_us[k], "bytes_per_launch": b_phase[k], "GBps": b_phase[k] / ph_us[k] / 1e3 if ph_us[k] > 0 else None} for k in range(3)},
                    "iteration": {"bytes_moved_model": sum(b_phase), "GBps": sum(b_phase) / ms / 1e6, "frac_hbm_peak": sum(b_phase) / ms / 1e6 / HBM_PEAK_GBS},
                    "final_rel_residual": float(gcr.last_history[-1])}
    c = out["complex_values_20B_per_entry"]
    out["roofline"] = {"kernel": "whole iteration (3 kernels), complex slab", "bound": "hbm", "achieved": c["iteration"]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": c["iteration"]["frac_hbm_peak"], "traffic": None, "bytes_per_launch": c["iteration"]["bytes_moved_model"]}
    return out


def make_unstructured_blocks(nb, bs, seed=5):
    """configs[4]'s operator: unstructured HierarchicalSparse, skewed blocks per row (80 % of the block rows
    5-9 blocks, 20 % 10-64), diagonally dominant."""
    import numpy as np
    rng = np.random.default_rng(seed)
    per_row = np.where(rng.random(nb) < 0.8, rng.integers(5, 10, nb), rng.integers(10, 65, nb))
    rows = np.repeat(np.arange(nb, dtype=np.int32), per_row)
    cols = rng.integers(0, nb, rows.size).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(per_row)[:-1]])
    cols[first] = np.arange(nb, dtype=np.int32)
    nblk = rows.size
    blocks = np.empty((nblk, bs, bs), np.complex128)
    for s in range(0, nblk, 20000):
        e = min(nblk, s + 20000)
        blocks[s:e] = (rng.uniform(-1, 1, (e - s, bs, bs)) + 1j * rng.uniform(-1, 1, (e - s, bs, bs))) * (0.5 / bs)
    offsum = np.bincount(rows, weights=np.abs(blocks).sum(axis=(1, 2)) / bs, minlength=nb)
    blocks[first] = np.eye(bs)[None] * (1.0 + offsum)[:, None, None]
    return rows, cols, blocks


def wl_bcsr_mg(args):
    """configs[4] as BASELINE states it, on one GPU: MG-preconditioned GCR on the ~3 GB unstructured HierarchicalSparse — aggregates
    of 4 consecutive block rows (mesh = block rows x block size, only the first dimension blocked), 4 near-null vectors, one
    coarse level (a HierarchicalSparse of 4 x 4 blocks, Galerkin product on the device), smoother 2 GCR sweeps, coarsest solve GCR
    to 1e-2 / 50 iterations, flexible outer GCR restart 5 to 1e-10.  Reference: src/HierarchicalSparse.h:101-161, src/MG.h:405-430."""
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, HierarchicalSparse, MG, MG_Param, Mesh
    mg.init(0)
    bs, nb, sub, ne = 20, int(os.environ.get("MGCR_BENCH_BCSR_ROWS", 36000)), 4, 4
    rows, cols, blocks = make_unstructured_blocks(nb, bs)
    nblk = rows.size
    H = HierarchicalSparse(nb, nb, rows, cols, blocks)
    del blocks
    n = nb * bs
    dims = (nb, bs)
    rng = np.random.default_rng(9)
    vecs = np.ones((ne, n), np.complex128)
    vecs[1:] += 0.5 * (rng.standard_normal((ne - 1, n)) + 1j * rng.standard_normal((ne - 1, n)))
    rhs, x, y = Field(dims).fill_rhs(2), Field(dims).set_zero(), Field(dims)
    t0 = time.perf_counter()
    prm = MG_Param(Mesh(dims), sub, ne, None, GCR(GCR_Param(0, 10, 50, 1e-2, False)), GCR(GCR_Param(0, 10, 2, 1e-30, False)), 1,
                   None, None, spacetime=[True, False], null_vectors=vecs)
    M = MG(H, prm)
    mg.lib().mgcr_synchronize()
    setup_s = time.perf_counter() - t0
    M(rhs, out=y)

    def cycle():
        mg.lib().mgcr_synchronize()
        t = time.perf_counter()
        M(rhs, out=y)
        mg.lib().mgcr_synchronize()
        return time.perf_counter() - t
    vc = stats(repeat_timed(cycle, min_total=0.2, min_reps=5, max_reps=30))
    outer = GCR(H, GCR_Param(0, 5, 200, 1e-10, False, None, M, flexible=True, check_every=2))
    timed_solve(mg, outer, rhs, x)
    sv = stats(repeat_timed(lambda: timed_solve(mg, outer, rhs, x), min_total=0.2, min_reps=3, max_reps=8))
    r = rhs - H(x)
    plain = GCR(H, GCR_Param(0, 5, 200, 1e-10, False, check_every=5))
    timed_solve(mg, plain, rhs, x)
    sp = stats(repeat_timed(lambda: timed_solve(mg, plain, rhs, x), min_total=0.2, min_reps=3, max_reps=8))
    b_apply = nblk * (bs * bs * 16 + 4) + (nb + 1) * 4 + 2 * n * 16
    # fine level of a cycle: 2 + 2 smoother sweeps (4 applies; the residual is the pre-smoother's recurrence residual) — lower bound of the bytes
    b_cycle_lb = 4 * b_apply
    return {"workload": "unstructured HierarchicalSparse (block-CSR, bs 20, 5-64 blocks/row, ~3 GB), 2-level MG V-cycle preconditioner (aggregates of 4 block "
                        "rows, 4 near-null vectors), flexible GCR restart 5 to 1e-10, 1 GPU (configs[4] as stated)",
            "parity": MG_PARITY_NOTE, "block_rows": nb, "bs": bs, "blocks": int(nblk), "matrix_GB": nblk * bs * bs * 16 / 1e9,
            "levels": [M.level_info(l) for l in range(2)], "mg_setup_seconds": setup_s, "vcycle_ms": vc["median"] * 1e3, "vcycle_timing_seconds": vc,
            "vcycle_bytes_lower_bound_fine_applies": b_cycle_lb, "vcycle_GBps_lower_bound": b_cycle_lb / vc["median"] / 1e9,
            "vcycle_frac_hbm_peak_lower_bound": b_cycle_lb / vc["median"] / 1e9 / HBM_PEAK_GBS,
            "outer_iterations": outer.last_iterations, "converged": outer.last_converged, "seconds_to_tol": sv["median"], "solve_timing_seconds": sv,
            "final_rel_residual": float(outer.last_history[-1]), "true_rel_residual": r.norm() / rhs.norm(),
            "unpreconditioned": {"iterations": plain.last_iterations, "seconds_to_tol": sp["median"], "timing_seconds": sp},
            "roofline": {"kernel": "V-cycle (lower bound: its 4 fine-level block-CSR applies)", "bound": "hbm", "achieved": b_cycle_lb / vc["median"] / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": b_cycle_lb / vc["median"] / 1e9 / HBM_PEAK_GBS, "traffic": None}}



def wl_sample(args):
    """configs[0] on the GPU: data/sample_matrix (3072 rows, 39 entries per row) through read_data, DiracOp k = 0.15, GCR restart 5
    to 1e-13 — the reference's own golden history G3 is the check (118 iterations)."""
    import gzip
    import shutil
    import tempfile
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, read_data
    mg.init(0)
    d = tempfile.mkdtemp()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "4x4parsed.txt.gz"), "rb") as fi, open(os.path.join(d, "4x4parsed.txt"), "wb") as fo:
        shutil.copyfileobj(fi, fo)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):   # read_data prints the reference's "File read is successful."
        D = read_data("4x4parsed.txt", directory=d)
    dirac = DiracOp(D, 0.15)
    g = np.load(os.path.join(ROOT, "tests", "golden", "sample_4x4.npz"))
    dims = (4, 4, 4, 4, 4, 3)
    rhs, x = Field(dims, g["gcr_rhs"]), Field(dims)
    gcr = GCR(dirac, GCR_Param(0, 5, 4000, 1e-13, False, check_every=20))
    timed_solve(mg, gcr, rhs, x)
    sv = stats(repeat_timed(lambda: timed_solve(mg, gcr, rhs, x), min_total=0.2, min_reps=10))
    ref = g["g3_restart5_hist"]
    h = gcr.last_history
    m = min(h.size, ref.size)
    return {"workload": "data/sample_matrix 4x4 (3072 rows), 1 - 0.15 D, GCR restart 5 to 1e-13 (configs[0] on the GPU)",
            "iterations": gcr.last_iterations, "reference_iterations": int(ref.size - 1), "seconds": sv["median"], "timing_seconds": sv,
            "it_per_s": gcr.last_iterations / sv["median"], "final_rel_residual": float(h[-1]), "reference_final": float(ref[-1]),
            "max_rel_deviation_from_reference_history": float(np.max(np.abs(h[1:m] - ref[1:m]) / ref[1:m])),
            "note": "latency regime: 3 dependent kernels per iteration on 3072 rows"}


def wl_latency64(args):
    """The latency regime: Poisson 64^3 (262 144 rows = the coarsest level of configs[2]'s hierarchy), GCR restart 10, 400 iterations
    — the one-launch resident solver (csrc/gcr_resident.hip) beside the multi-kernel path on the same operator; both must give the
    same residual to the last bit."""
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, Sparse, problems
    mg.init(0)
    n, restart, its = 64, 10, 400
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    A = Sparse(N, ncol, rowptr, col, val)
    dims = (n, n, n)
    rhs = Field(dims).fill_rhs(0)
    out = {}
    for resident in (1, 0):
        prev = mg.set_option("resident_solver", resident)
        try:
            g = GCR(A, GCR_Param(0, restart, its, 1e-300, False))
            x = Field(dims)
            before = mg.stat("resident_solves")
            timed_solve(mg, g, rhs, x)
            took = mg.stat("resident_solves") - before

            sv = stats(repeat_timed(lambda: timed_solve(mg, g, rhs, x), min_total=0.1, min_reps=5))
            out["resident" if resident else "multi_kernel"] = {
                "us_per_iteration": sv["median"] * 1e6 / g.last_iterations, "it_per_s": g.last_iterations / sv["median"], "timing_seconds": sv,
                "iterations": g.last_iterations, "final_rel_residual": float(g.last_history[-1]), "one_launch_path_taken": bool(took)}
        finally:
            mg.set_option("resident_solver", prev)
    return {"workload": "latency regime: 3D 7-point Poisson 64^3, GCR restart 10, 400 iterations, fp64", **out,
            "same_residual_bits": out["resident"]["final_rel_residual"] == out["multi_kernel"]["final_rel_residual"],
            "speedup": out["multi_kernel"]["us_per_iteration"] / out["resident"]["us_per_iteration"]}


def wl_poisson128_tol(args):
    """configs[1] run to tolerance (not in the default line: it takes a second or so): GCR restart 5 to 1e-13 on Poisson
    128^3, and the same solve with configs[2]'s 3-level MG as flexible right preconditioner."""
    import numpy as np
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Field, GCR, GCR_Param, MG, MG_Param, Mesh, Sparse, problems
    mg.init(0)
    n, tol = 128, 1e-13
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    A = Sparse(N, ncol, rowptr, col, val)
    del rowptr, col, val
    dims = (n, n, n)
    rhs, x = Field(dims).fill_rhs(0), Field(dims)
    gcr = GCR(A, GCR_Param(0, 5, 200000, tol, False, check_every=50))
    timed_solve(mg, gcr, rhs, x)
    dt = timed_solve(mg, gcr, rhs, x)
    out = {"workload": "3D 7-point Poisson 128^3, GCR restart 5 to 1e-13 (time to tolerance), then MG-preconditioned", "tol": tol,
           "iterations": gcr.last_iterations, "converged": gcr.last_converged, "seconds_to_tol": dt, "it_per_s": gcr.last_iterations / dt,
           "true_rel_residual": (rhs - A(x)).norm() / rhs.norm()}
    t0 = time.perf_counter()
    prm = MG_Param(Mesh(dims), 2, 1, None, GCR(GCR_Param(0, 10, 50, 1e-2, False)), GCR(GCR_Param(0, 10, 2, 1e-30, False)),
                   2, None, None, null_vectors=np.ones((1, N), np.complex128))
    M = MG(A, prm)
    mg.lib().mgcr_synchronize()
    out["mg_setup_seconds"] = time.perf_counter() - t0
    outer = GCR(A, GCR_Param(0, 5, 500, tol, False, None, M, flexible=True, check_every=2))
    timed_solve(mg, outer, rhs, x)
    dt = timed_solve(mg, outer, rhs, x)
    out.update(mg_parity=MG_PARITY_NOTE, mg_outer_iterations=outer.last_iterations, mg_converged=outer.last_converged, mg_seconds_to_tol=dt,
               mg_true_rel_residual=(rhs - A(x)).norm() / rhs.norm())
    return out


# ------------------------------------------------------------------------------------------------
# N > 1 only: BASELINE configs[3] and configs[4] in their multi-GPU form (worker processes of the supervisors, started
# after the headline with the transport that carried it; MGCR_BENCH_WORKLOAD selects one)
# ------------------------------------------------------------------------------------------------
def dist_context():
    """What every distributed worker sets up: device, gloo control plane, the library's communicator."""
    import torch
    import torch.distributed as dist
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import Comm
    rank, world, local_rank = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    one_gpu = os.environ.get("MGCR_BENCH_ONE_GPU", "0") == "1"
    host_transport = os.environ.get("MGCR_BENCH_TRANSPORT", "rccl") == "host" or one_gpu
    torch.cuda.set_device(0 if one_gpu else local_rank)
    mg.init(0 if one_gpu else local_rank)
    dist.init_process_group("gloo", init_method=worker_init_method(), rank=rank, world_size=world)
    if host_transport:
        comm = Comm.host(dist)
    else:
        try:
            comm, err = Comm.rccl(dist), None
        except Exception as e:  # noqa: BLE001
            comm, err = None, repr(e)
        bad = torch.tensor([0 if err is None else 1], dtype=torch.int32)
        dist.all_reduce(bad)
        if int(bad[0]):
            raise SystemExit("RCCL communicator creation failed on %d rank(s): %s" % (int(bad[0]), err))

    def timed(fn):
        """wall seconds of fn(), barrier + synchronise on both sides, max over ranks"""
        mg.lib().mgcr_synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        fn()
        mg.lib().mgcr_synchronize()
        dt = time.perf_counter() - t0
        dist.barrier()
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0])

    def teardown():
        dist.barrier()
        mg.lib().mgcr_synchronize()
        mg.lib().mgcr_comm_destroy(comm.h)
        comm.h = None
        dist.destroy_process_group()
        mg.finalize()
    return rank, world, comm, timed, teardown, ("host-staged" if host_transport else "RCCL") + (", all ranks on GPU 0 (rehearsal, not a result)" if one_gpu else "")


def wl_dist_mg(args):
    """configs[3]: 3-D 7-point Poisson, slab-partitioned, 64 planes of 512 x 512 per GPU (512^3 on 8 GPUs), 3-level aggregation
    MG built collectively (2^3 aggregates inside the slab, Galerkin across the slab boundaries, distributed coarse
    operators) as flexible right preconditioner of GCR restart 5 to 1e-8."""
    import numpy as np
    from mgpreconditionedgcr_amd import DistSparse, Field, GCR, GCR_Param, MG, MG_Param, Mesh, problems
    rank, world, comm, timed, teardown, transport = dist_context()
    n, planes, tol = int(os.environ.get("MGCR_BENCH_DIST_N", "512")), int(os.environ.get("MGCR_BENCH_DIST_PLANES", "64")), 1e-8
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n, rank * planes, (rank + 1) * planes, ni=world * planes)
    A = DistSparse(comm, ncol, rank * N, rowptr, col, val)
    del rowptr, col, val
    dims = (planes, n, n)
    rhs, x, y = Field(dims).fill_rhs(0, global_offset=rank * N), Field(dims), Field(dims)
    prm = MG_Param(Mesh(dims), 2, 1, None, GCR(GCR_Param(0, 10, 50, 1e-2, False)), GCR(GCR_Param(0, 10, 2, 1e-30, False)),
                   2, None, None, null_vectors=np.ones((1, N), np.complex128))
    box = {}
    setup_s = timed(lambda: box.setdefault("M", MG(A, prm)))
    M = box["M"]
    M(rhs, out=y)
    vc = stats([timed(lambda: M(rhs, out=y)) for _ in range(5)])
    outer = GCR(A, GCR_Param(0, 5, 200, tol, False, None, M, flexible=True, check_every=2))

    def solve():
        x.set_zero()
        outer.solve(rhs, x)
    solve()
    sv = stats([timed(solve) for _ in range(3)])
    r = rhs - A(x)
    true_rel = float(np.sqrt(comm.dot(r, r).real / comm.dot(rhs, rhs).real))
    out = {"workload": "3D 7-point Poisson (%d x %d x %d), slab x%d, 3-level MG V-cycle preconditioner, flexible GCR restart 5 to 1e-8, fp64 "
                       "(configs[3]%s)" % (world * planes, n, n, world, "" if (n, planes, world) != (512, 64, 8) else ": 512^3 on 8 GPUs"),
           "parity": MG_PARITY_NOTE, "n_gpus": world, "rows_per_gpu": N, "rows": N * world, "transport": transport,
           "halo_kind": A.halo_kind, "allreduce_kind": comm.allreduce_kind, "levels_local": [M.level_info(l) for l in range(3)],
           "mg_setup_seconds": setup_s, "vcycle_ms": vc["median"] * 1e3, "vcycle_timing_seconds": vc,
           "outer_iterations": outer.last_iterations, "converged": outer.last_converged, "seconds_to_tol": sv["median"],
           "solve_timing_seconds": sv, "tol": tol, "final_rel_residual": float(outer.last_history[-1]), "true_rel_residual": true_rel}
    del outer, M, A, x, y, rhs, r
    teardown()
    return out


def wl_dist_bcsr(args):
    """configs[4]: unstructured HierarchicalSparse distributed by block rows (bs 20, 5-64 blocks per row, block columns
    anywhere on any rank, ~3 GB of blocks per GPU, diagonally dominant): apply with the block-granular halo, GCR restart 5
    to 1e-10 on it."""
    import numpy as np
    from mgpreconditionedgcr_amd import DistHierarchicalSparse, Field, GCR, GCR_Param
    rank, world, comm, timed, teardown, transport = dist_context()
    bs, nbl = 20, int(os.environ.get("MGCR_BENCH_DIST_NB", "36000"))
    nbg = nbl * world
    rng = np.random.default_rng(5 + rank)
    per_row = np.where(rng.random(nbl) < 0.8, rng.integers(5, 10, nbl), rng.integers(10, 65, nbl))
    rows = np.repeat(np.arange(nbl, dtype=np.int64), per_row)
    cols = rng.integers(0, nbg, rows.size).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(per_row)[:-1]])
    cols[first] = rank * nbl + np.arange(nbl, dtype=np.int64)       # the diagonal block of every row
    nblk = rows.size
    blocks = np.empty((nblk, bs, bs), np.complex128)
    for s in range(0, nblk, 20000):
        e = min(nblk, s + 20000)
        blocks[s:e] = (rng.uniform(-1, 1, (e - s, bs, bs)) + 1j * rng.uniform(-1, 1, (e - s, bs, bs))) * (0.5 / bs)
    offsum = np.bincount(rows, weights=np.abs(blocks).sum(axis=(1, 2)) / bs, minlength=nbl)
    blocks[first] = np.eye(bs)[None] * (1.0 + offsum)[:, None, None]
    H = DistHierarchicalSparse(comm, nbg, rank * nbl, nbl, rows, cols, blocks)
    del blocks
    n = nbl * bs
    xf, yf = Field((n,)).fill_rhs(1, global_offset=rank * n), Field((n,))
    H(xf, out=yf)
    ap = stats([timed(lambda: [H(xf, out=yf) for _ in range(10)]) / 10 for _ in range(5)])
    b_alg = nblk * (bs * bs * 16 + 4) + (nbl + 1) * 4 + 2 * n * 16
    rhs, x = Field((n,)).fill_rhs(2, global_offset=rank * n), Field((n,))
    gcr = GCR(H, GCR_Param(0, 5, 200, 1e-10, False, check_every=5))

    def solve():
        x.set_zero()
        gcr.solve(rhs, x)
    solve()
    sv = stats([timed(solve) for _ in range(3)])
    r = rhs - H(x)
    true_rel = float(np.sqrt(comm.dot(r, r).real / comm.dot(rhs, rhs).real))
    out = {"workload": "unstructured HierarchicalSparse distributed by block rows over %d GPUs (bs 20, 5-64 blocks/row, columns on any rank), "
                       "apply + GCR restart 5 to 1e-10 (configs[4]'s operator)" % world,
           "n_gpus": world, "block_rows_per_gpu": nbl, "blocks_per_gpu": int(nblk), "matrix_GB_per_gpu": nblk * bs * bs * 16 / 1e9,
           "transport": transport, "halo_kind": H.halo_kind, "allreduce_kind": comm.allreduce_kind,
           "apply_ms_incl_halo_exchange": ap["median"] * 1e3, "apply_timing_seconds": ap, "algorithmic_bytes_per_gpu": b_alg,
           "GBps_per_gpu": b_alg / ap["median"] / 1e9, "frac_hbm_peak_per_gpu": b_alg / ap["median"] / 1e9 / HBM_PEAK_GBS,
           "gcr_iterations": gcr.last_iterations, "gcr_converged": gcr.last_converged, "gcr_seconds": sv["median"], "gcr_timing_seconds": sv,
           "true_rel_residual": true_rel}
    del gcr, H, x, rhs, xf, yf, r
    teardown()
    return out


DIST_WORKLOADS = {"dist_mg": wl_dist_mg, "dist_bcsr": wl_dist_bcsr}
DIST_EXTRA_TIMEOUT_S = 240

WORKLOADS = {"poisson128_tol": wl_poisson128_tol, "poisson256_gcr": wl_poisson256_gcr, "poisson512_gcr": wl_poisson512_gcr, "mg256": wl_mg256, "mg512": wl_mg512, "ell_slab_spmv128": wl_ell_slab_spmv128, "bcsr": wl_bcsr,
             "sample": wl_sample, "latency64": wl_latency64, "irregular_spmv": wl_irregular_spmv, "poisson128_gcr_general": wl_poisson128_gcr_general,
             "bcsr_mg": wl_bcsr_mg}


def run_extras(argv_base, budget_s=420.0):
    """Every other workload in its own child process (python bench.py --workload NAME), bounded in time."""
    out = {}
    t_end = time.time() + budget_s
    for name in EXTRA_WORKLOADS:
        left = t_end - time.time()
        if left < 20:
            out[name] = {"skipped": "time budget of the default run used up"}
            continue
        env = dict(os.environ, MGCR_BENCH_ROLE="worker")
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name], env=env, capture_output=True, text=True,
                               timeout=min(left, 150))
            d = last_json_line(p.stdout)
            out[name] = d if (p.returncode == 0 and d is not None) else {"failed": "rc %d" % p.returncode, "stderr_tail": p.stderr[-500:]}
        except subprocess.TimeoutExpired:
            out[name] = {"failed": "timeout"}
    return out


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--grid", dest="n", type=int, default=128, help="Poisson grid edge per GPU shard (128 = BASELINE configs[1])")
    ap.add_argument("--restart", type=int, default=5)
    ap.add_argument("--spmv-reps", type=int, default=50)
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: repeated solves, per-phase timings, SpMV and roofline figures, CPU baselines and the "
                         "other configs' workloads")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the other configs' workloads")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed solve computed (x, residual history; N > 1: rank 0's shard of x) as DIR/<name>.npy")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="run ONE of the other workloads in this process and print its JSON")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.workload:
        print(json.dumps(WORKLOADS[args.workload](args)), flush=True)
        return 0
    role = os.environ.get("MGCR_BENCH_ROLE")
    world_env = os.environ.get("WORLD_SIZE")
    if role == "worker":
        wl = os.environ.get("MGCR_BENCH_WORKLOAD")
        out = DIST_WORKLOADS[wl](args) if wl else run_headline(args, with_cpu=False)
        if int(os.environ.get("RANK", "0")) == 0:
            print(json.dumps(out), flush=True)
        return 0
    if args.gpus > 1 and world_env is None:
        os.environ["MGCR_BENCH_STARTED_BY"] = "bench.py launcher"
        return run_launcher(args, argv)
    world = int(world_env or "1")
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world > 1:
        return run_supervisor(args, argv)
    try:
        out = run_headline(args, with_cpu=not args.no_cpu_baseline)
    except Exception as e:
        # The one-launch paths (csrc/gcr_stepbuild.hip, gcr_resident.hip) need their workgroups co-resident; if foreign work
        # on the device made one give up (bounded polls -> error, never a hang), a line from the three-kernel path beats none.
        if "co-resident" not in str(e):
            raise
        import mgpreconditionedgcr_amd as mg
        mg.lib().mgcr_synchronize()
        mg.set_option("step_build", 0)
        mg.set_option("resident_solver", 0)
        os.environ["MGCR_STEPBUILD"] = "0"      # the workloads' child processes as well
        os.environ["MGCR_RESIDENT"] = "0"
        out = run_headline(args, with_cpu=not args.no_cpu_baseline)
        out["fallback"] = "one-launch paths switched off after: %s" % (str(e)[:300],)
    if args.full and not args.no_extras:
        out["workloads"] = run_extras(argv)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
