"""Headline benchmark: converged eigenpairs/sec (k=20, shift-invert) + SpMV HBM GB/s vs roofline  (BASELINE.json).

One "step" = one complete shift-invert eigensolve of the synthetic cylinder pair (A, M) that is already resident in
HBM: build C = A - sigma M on the device, factorise it, Krylov-Schur (ncv = 80) with one inner solve per Arnoldi step,
until k = 20 pairs pass the relative-residual test.  A pair counts as converged iff
||A v - lam M v|| / (||A v|| + |lam| ||M v||) <= 1e-8 (formula of Solver/eigen2.py:48-56), checked on the device after
the timed region.

Inner solve (--pc): "lu" (default, the reference's own setting, .examples/eigenvalues.py:100) = exact nested-dissection
multifrontal LU on the device, every solve verified against b - C x and wrapped in GMRES; "ilu" = ILU(k)-preconditioned
GMRES with the blocked SpTRSV (the north-star variant).  The headline `value` is the --pc run; with --full the other variant is
timed once and reported under config.other_pc.

    python bench.py --gpus 1 --steps 2 --warmup 1                  # the headline only
    python bench.py --gpus 1 --steps 2 --warmup 1 --full           # + every secondary figure below
    python bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

N > 1 (one rank per GPU): `value` is the SAME workload as at N = 1 -- every rank solves the S30k problem on its own GPU, no
data-path collective ("weak": per-GPU work fixed, the driver's 1 -> 8 curve compares one problem with itself); `--sweep` gives
each rank its own shift of the reference's Re-sweep table (.examples/eigenvalues.py:37-49) instead.  The layout BASELINE.json's
north_star names -- ONE problem, the 500 k-unknown pair of config 3, row-sharded over the ranks with RCCL all-gathers over
xGMI -- is measured in the same run as `config.sharded`: every rank starts a child process (`--sharded-child`) that joins a
process group of its own; the children cut the nested-dissection forest of C = A - sigma M over the ranks (own subtrees, one
in-place all-gather of the subtree roots' update matrices, replicated top; Krylov bases replicated; an operator apply = the
exact solve of the one-GPU path with two all-gathers), solve once with one Arnoldi step per read-back and once with the
batched steps and compare the eigenvalues, time the steps, and time the same problem on ONE GPU beside it
(`one_gpu_same_workload_eigenpairs_per_s`, with --full).  The children run under a time limit (`--sharded-timeout`): the multi-rank RCCL
exchange has never run on hardware available to the build, and a fault or hang there must cost `config.sharded`, not the
bench line.  `--layout sharded` makes the sharded run the headline instead (strong scaling, S500k).  Rehearsal on one GPU:
tools/rehearse_two_ranks.sh (LSA_BENCH_DEVICE=0 LSA_BENCH_BACKEND=gloo: all ranks on device 0, host-staged all-gather).

Set-up (untimed): assembly, prepare() (ordering, upload, pattern analysis) and the process's first two solves (one-time costs
of kernel loading and of the runtime); then W warm-up steps, then K timed steps between barriers.  What the
set-up costs is on the line: `config.prepare_ms`, `config.analysis_ms`, `config.cold_first_solve_ms` (prepare + the process's
first solve: what a caller with ONE eigenproblem pays), `config.setup_solves`.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, the result line.  Everything else is measured
with --full only: config.other_pc, the solves in flight, config.lu_apply (and config.analysis_ms), config.sptrsv_roofline,
config.pattern_3d, `roofline`, `cpu_baseline`, and at N > 1 config.sharded_3d and config.replicas of the sharded layout.
--dump-outputs DIR writes what the last timed step returned (rank 0): eigenvalues.npy (k, 2) and eigenvectors.npy (k, n, 2),
float64 with a trailing (re, im) axis; the inputs are deterministic, so two builds can be compared output for output.

Rank 0 prints ONE JSON line.  `roofline` is measured on the SpMV kernel (the kernel the metric names) on SROOF, a
~1.5e8-nnz CSR with the cylinder-flow row pattern that does not fit the 256 MB Infinity Cache; `cpu_baseline` is the
oracle (scipy ARPACK + SuperLU, the algorithm Solver/eigen2.py states) on the same S30k problem on the host cores (N = 1 only).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

# Host BLAS on one thread (unless the caller chose otherwise).  Measured on the GPU box (tools/micro/after_solve.py,
# DESIGN.md section 6): numpy's 64 OpenBLAS workers keep spinning for ~0.1 s after any threaded call (a 30k-entry norm
# is enough); on the 16-core share of a one-GPU box that starves the HIP runtime's helper thread and the next
# factorisation's 3 900 dependent launches take 88-144 ms instead of 66.  It also is the honest setting for the CPU
# baseline: single-threaded SuperLU/ARPACK ran 5x FASTER with one BLAS thread than with 64 (6 s vs 30 s per solve).
for _var in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS", "LSA_HOST_BLAS_THREADS"):
    os.environ.setdefault(_var, "1")
# one solve drives up to four streams; the secondary "two solves in flight" figure needs a second set of hardware queues
# (the runtime's default is four per process; read when the first HIP context is created)
if int(os.environ.get("WORLD_SIZE", "1")) == 1:  # (with several processes on one GPU, as in the one-box rehearsal of
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # N > 1, more than 8 queues per GPU in total slow everything down)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

# Re = 40..90 shifts of the reference sweep; index 2 is Re = 50
SWEEP_SIGMAS = (
    -0.03 + 0.7197388769374216j, 0.7316769290210628j, 0.018 + 0.7379601143282424j, 0.03 + 0.742986662573986j,
    0.05 + 0.744243299635422j, 0.061 + 0.7461282552275759j, 0.072 + 0.7461282552275759j, 0.085 + 0.744557458900781j,
)
RESIDUAL_TOL = 1e-8
HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md


def log(msg: str) -> None:
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


if os.environ.get("LSA_BENCH_STACKS"):  # development: python stacks of every thread to stderr every N seconds (finding a hang)
    import faulthandler

    faulthandler.dump_traceback_later(float(os.environ["LSA_BENCH_STACKS"]), repeat=True, file=sys.stderr)


def build_solver(es, sigma, args, device, pc, layout="single"):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    cfg = EigensolverConfig(num_eig=args.k, atol=args.atol, ncv=args.ncv, max_it=500)
    kw = {"ilu_levels": args.ilu_levels} if pc == "ilu" else {}
    solver = EigenSolver(es.A, es.M, cfg, check_hermitian=False, restart=args.restart, device=device, layout=layout, **kw)
    solver.solver.set_st_type(iSTType.SINVERT)
    solver.solver.set_target(sigma)
    solver.solver.set_st_pc_type(PreconditionerType.ILU if pc == "ilu" else PreconditionerType.LU)
    return solver


def spmv_roofline(args, device):
    """SpMV on SROOF: achieved algorithmic GB/s from HIP-event time per launch (library stream)."""
    import lsa_hip
    from synthetic import fem
    from Solver.utils import pivot_safe_rcm

    t0 = time.time()
    es = fem.cylinder_case(args.roof_case)
    C = sp.csr_matrix((es.A.data - fem.SIGMA_RE50 * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    perm = pivot_safe_rcm(C)
    C = C[perm][:, perm].tocsr()
    C.sort_indices()
    n1, nnz1, reps = C.shape[0], C.nnz, args.roof_reps
    # block-diagonal replicas: same row-degree histogram and column locality, footprint beyond the Infinity Cache
    rp = np.concatenate([[0], (C.indptr[1:][None, :] + (np.arange(reps) * nnz1)[:, None]).ravel()]).astype(np.int32)
    ci = (C.indices[None, :] + (np.arange(reps, dtype=np.int64) * n1)[:, None]).ravel().astype(np.int32)
    val = np.tile(C.data, reps)
    big = sp.csr_matrix((val, ci, rp), shape=(n1 * reps, n1 * reps))
    n, nnz = big.shape[0], big.nnz
    log(f"SROOF = {reps} x {args.roof_case}: n={n} nnz={nnz} ({(20 * nnz + 36 * n) / 1e9:.2f} GB algorithmic, c128) built in {time.time() - t0:.1f}s")
    ctx = lsa_hip.Context(device)
    out = {}
    try:
        rng = np.random.default_rng(0)
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        dC = lsa_hip.CsrMatrix.from_scipy(ctx, big)
        dx = lsa_hip.DeviceVector.from_numpy(ctx, x)
        dy = lsa_hip.DeviceVector(ctx, n, np.complex128)
        dC.time_matvec(dx, dy, 5)
        ms = dC.time_matvec(dx, dy, args.roof_iters)
        bytes_c = 20.0 * nnz + 36.0 * n  # 16 B value + 4 B column per entry; 4 B rowptr + 16 B x + 16 B y per row
        info = dC.matvec_info(np.complex128)  # the kernel lsa_spmv really launched and the bytes THAT kernel moves
        out["c128"] = {"ms": ms, "bytes": bytes_c, "gbs": bytes_c / ms / 1e6, "kernel": info["kernel"], "moved": float(info["bytes_moved"]),
                       "moved_gbs": info["bytes_moved"] / ms / 1e6}
        # the f64 variant of the same pattern (real sigma path): 12 nnz + 20 n bytes
        bigr = sp.csr_matrix((np.ascontiguousarray(val.real), ci, rp), shape=big.shape)
        del dC
        dR = lsa_hip.CsrMatrix.from_scipy(ctx, bigr)
        dxr = lsa_hip.DeviceVector.from_numpy(ctx, x.real.copy())
        dyr = lsa_hip.DeviceVector(ctx, n, np.float64)
        dR.time_matvec(dxr, dyr, 5)
        msr = dR.time_matvec(dxr, dyr, args.roof_iters)
        bytes_r = 12.0 * nnz + 20.0 * n
        infor = dR.matvec_info(np.float64)
        out["f64"] = {"ms": msr, "bytes": bytes_r, "gbs": bytes_r / msr / 1e6, "kernel": infor["kernel"]}
        out["n"], out["nnz"] = n, nnz
        del dR, dx, dy, dxr, dyr
    finally:
        import gc

        gc.collect()
        ctx.close()
    return out


def pmc_traffic(args, kernel: str):
    """HBM bytes per SpMV launch from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled per the gfx950 note of
    MI355X_MICROARCH.md, + WRITE_SIZE); PMC counters cannot be collected inside this process.  None unless the committed
    profile is for this SROOF configuration AND for the kernel this run launched (name and template arguments)."""
    if args.roof_case != "S500k" or args.roof_reps != 10:
        return None
    squash = lambda t: "".join(t.split()).replace("void", "")  # noqa: E731
    for path in sorted((ROOT / "profiles").glob("r*_spmv_traffic.json"), reverse=True):
        rec = json.loads(path.read_text()).get("c128", {})
        if squash(kernel) and squash(rec.get("kernel", "")).startswith(squash(kernel)):
            return float(rec["traffic_bytes"])
    return None


def solves_in_flight(es, sigma, args, device, jobs=2, rounds=4):
    """Secondary figure (not `value`): `jobs` independent solves of the same problem in flight on ONE GPU, one Python
    thread + HIP context + stream set each -- what `examples/eigenvalues.py --jobs` does for a Reynolds sweep.  A single
    solve is a chain of dependent launches and leaves most of the GPU idle."""
    import threading

    solvers = [build_solver(es, sigma, args, device, args.pc) for _ in range(jobs)]
    for so in solvers:
        so.solver.prepare()
        so.solve()
    pairs = [0] * jobs
    bits = [set() for _ in range(jobs)]  # the eigenvalues every solve returned, as bit patterns

    def work(j):
        for _ in range(rounds):
            so = solvers[j]
            got = so.solve()
            pairs[j] += int(np.sum(so.solver.residuals()[: args.k] <= RESIDUAL_TOL))
            bits[j].add(np.array([p[0] for p in got[: args.k]], dtype=np.complex128).tobytes())

    threads = [threading.Thread(target=work, args=(j,)) for j in range(jobs)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    for so in solvers:
        so.solver.release()
    return {"jobs": jobs, "eigenpairs_per_s": sum(pairs) / dt, "ms_per_round": 1e3 * dt / rounds,
            # solves that overlap on the GPU must return the bits of a solve that has the GPU to itself
            "bit_identical_eigenvalues": len(set().union(*bits)) == 1,
            "note": "secondary: independent solves overlapped on one GPU (threads); `value` is one solve at a time"}


def ordered_for_lu(C):
    """What Solver/utils.py::prepare does before an exact-LU solve: the matrix in the elimination order of the nested
    dissection, the forest handed back to the library (vectors in that order: the sweeps address own unknowns without index lists)."""
    import lsa_hip

    zd = C.diagonal() == 0
    o = lsa_hip.nd_order(C, 0, constraint=zd if (zd.any() and C.nnz > 60 * C.shape[0]) else None)
    Cp = C[o["perm"]][:, o["perm"]].tocsr()
    Cp.sort_indices()
    return Cp, {"first": o["first"], "size": o["size"], "parent": o["parent"]}


def lu_apply_rate(es, sigma, device):
    """Secondary figure: one inner solve of the exact LU (upward + downward sweep over the elimination forest),
    HIP-event time per apply against its algorithmic bytes (every factor scalar once + the vectors: lsa_ndlu_info), and
    the numeric refactorisation time for a new shift on the analysed pattern."""
    import lsa_hip

    C, tree = ordered_for_lu(sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape))
    ctx = lsa_hip.Context(device)
    try:
        dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
        f = lsa_hip.NdLu(ctx, dC, tree=tree)
        rng = np.random.default_rng(0)
        db = lsa_hip.DeviceVector.from_numpy(ctx, rng.standard_normal(es.n) + 1j * rng.standard_normal(es.n))
        dx = lsa_hip.DeviceVector(ctx, es.n, np.complex128)
        f.time_solve(db, dx, 10)
        ms = f.time_solve(db, dx, 200)
        f.refactor(dC)
        info = f.info()
        out = {"ms_per_apply": ms, "algorithmic_bytes": info["apply_bytes"], "achieved_GBps": info["apply_bytes"] / ms / 1e6,
               "frac_of_hbm_peak": info["apply_bytes"] / ms / 1e6 / HBM_PEAK_GBS, "tree_nodes": info["tree_nodes"], "tree_levels": info["levels"],
               "max_front": info["max_front"], "dependent_launches": info["apply_launches"], "seconds_analyse": info["seconds_analyse"],
               "seconds_refactor": info["seconds_numeric"]}
        f = db = dx = dC = None
    finally:
        import gc

        gc.collect()
        ctx.close()
    return out


def _slepc_reference(es, sigma, args):
    """Row B1 of BASELINE.md: the reference's own stack (slepc4py Krylov-Schur, ST sinvert, -st_pc_type lu) when the box has it.
    The GPU boxes receive only this repository, so this normally reports that SLEPc is absent."""
    try:
        from petsc4py import PETSc
        from slepc4py import SLEPc
    except Exception as exc:  # noqa: BLE001
        return {"available": False, "why": f"{type(exc).__name__}: {exc}"}
    A, M = es.A.astype(np.complex128), es.M.astype(np.complex128)
    pA = PETSc.Mat().createAIJ(size=A.shape, csr=(A.indptr, A.indices, A.data))
    pM = PETSc.Mat().createAIJ(size=M.shape, csr=(M.indptr, M.indices, M.data))
    eps = SLEPc.EPS().create()
    eps.setOperators(pA, pM)
    eps.setProblemType(SLEPc.EPS.ProblemType.GNHEP)
    eps.setDimensions(args.k, args.ncv)
    eps.setTolerances(args.atol, 500)
    eps.setTarget(sigma)
    eps.setWhichEigenpairs(SLEPc.EPS.Which.TARGET_MAGNITUDE)
    st = eps.getST()
    st.setType(SLEPc.ST.Type.SINVERT)
    st.getKSP().setType("preonly")
    st.getKSP().getPC().setType("lu")
    t0 = time.perf_counter()
    eps.solve()
    dt = time.perf_counter() - t0
    return {"available": True, "eigenpairs_per_s": min(eps.getConverged(), args.k) / dt, "seconds": dt,
            "lambda": [complex(eps.getEigenvalue(i)) for i in range(min(eps.getConverged(), args.k))]}


def _cpu_worker(args) -> None:
    """Child process of cpu_baseline (no GPU): one oracle solve with the BLAS thread count of its environment."""
    from oracle import shift_invert
    from synthetic import fem

    es = fem.cylinder_case(args.case)
    sigma = SWEEP_SIGMAS[2]
    t0 = time.perf_counter()
    lam, V, res, info = shift_invert.solve(es.A, es.M, sigma, k=args.k, tol=args.atol, ncv=args.ncv, return_info=True)
    dt = time.perf_counter() - t0
    print(json.dumps({"seconds": dt, "eigenpairs_per_s": int(np.sum(res <= RESIDUAL_TOL)) / dt, "factor": info["seconds_factor"],
                      "applies": info["op_applies"], "lam": [[z.real, z.imag] for z in lam]}), flush=True)


def cpu_baseline(es, sigma, args):
    """The oracle (scipy ARPACK + SuperLU, the algorithm Solver/eigen2.py states) on the same problem, same k / ncv /
    tolerance, on the host cores: once with one BLAS thread and once with 8 (each in a child process started with that
    thread count: resizing a live OpenBLAS pool under SuperLU crashed); the faster run is the baseline.  SuperLU itself is
    sequential; more BLAS threads were measured slower on these supernode sizes.  A slepc4py run is added when the box has it."""
    import subprocess

    runs = []
    for threads in (1, 8):
        env = dict(os.environ)
        for var in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):
            env[var] = str(threads)
        env["HIP_VISIBLE_DEVICES"] = ""  # the checker never touches the GPU
        cmd = [sys.executable, str(ROOT / "bench.py"), "--cpu-worker", "--case", args.case, "--k", str(args.k), "--ncv", str(args.ncv), "--atol", str(args.atol)]
        try:
            proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            rec = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
        except Exception as exc:  # noqa: BLE001
            log(f"cpu baseline with {threads} thread(s) failed: {type(exc).__name__}: {exc}")
            continue
        rec["threads"] = threads
        runs.append(rec)
    if not runs:
        raise RuntimeError("no CPU baseline run finished")
    best = max(runs, key=lambda r: r["eigenpairs_per_s"])
    slepc = _slepc_reference(es, sigma, args)
    out = {
        # (SuperLU and ARPACK are sequential: one core does the work; the BLAS pool size of the faster run is reported beside it)
        "value": best["eigenpairs_per_s"], "unit": "eigenpairs/s", "cores": 1, "cores_used": 1, "blas_threads": best["threads"], "kind": "port",
        "sample": f"one full solve of the same {args.case} problem (k={args.k}, ncv={args.ncv}, tol={args.atol:g}) per thread count, scipy "
                  f"ARPACK+SuperLU: " + "; ".join(f"{r['threads']} BLAS thread(s) {r['seconds']:.1f} s (SuperLU factor {r['factor']:.1f} s, "
                                                  f"{r['applies']} applies)" for r in runs)
                  + f"; host has {os.cpu_count()} cores; slepc4py: " + ("ran" if slepc.get("available") else "not installed"),
        "runs": [{k: v for k, v in r.items() if k != "lam"} for r in runs],
    }
    if slepc.get("available"):
        out["slepc"] = {"eigenpairs_per_s": slepc["eigenpairs_per_s"], "seconds": slepc["seconds"]}
    return out, np.array([complex(a, b) for a, b in best["lam"]])


def sptrsv_roofline(args, device):
    """The sparse triangular solves of the exact LU (upward + downward sweep over the elimination forest = L and U solve) on
    the factors of the refined mesh S500k: HIP-event time per pair against the algorithmic bytes (every factor scalar once +
    the vectors).  SURVEY 8(d)'s figure for an ILU(0) pair, (20 nnz + 52 n) bytes of the UNfactored matrix, is given beside it."""
    import lsa_hip
    from synthetic import fem

    es = fem.cylinder_case(args.roof_case)
    C, tree = ordered_for_lu(sp.csr_matrix((es.A.data - fem.SIGMA_RE50 * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape))
    ctx = lsa_hip.Context(device)
    try:
        dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
        f = lsa_hip.NdLu(ctx, dC, tree=tree)
        rng = np.random.default_rng(0)
        b = rng.standard_normal(es.n) + 1j * rng.standard_normal(es.n)
        db = lsa_hip.DeviceVector.from_numpy(ctx, b)
        dx = lsa_hip.DeviceVector(ctx, es.n, np.complex128)
        f.time_solve(db, dx, 5)
        ms = f.time_solve(db, dx, 50)
        resid = float(np.linalg.norm(C @ dx.numpy() - b) / np.linalg.norm(b))
        f.refactor(dC)
        info = f.info()
        out = {"case": args.roof_case, "n": es.n, "nnz": int(C.nnz), "kernel": "nd_fwd_kernel + nd_bwd_kernel<cplx,cplx> (one launch per forest level and sweep)",
               "ms_per_pair": ms, "algorithmic_bytes": info["apply_bytes"], "achieved": info["apply_bytes"] / ms / 1e6, "unit": "GB/s",
               "frac": info["apply_bytes"] / ms / 1e6 / HBM_PEAK_GBS, "dependent_launches": info["apply_launches"], "factor_scalars": info["factor_entries"],
               "seconds_refactor": info["seconds_numeric"], "relative_residual": resid,
               "ilu0_pair_bytes_of_the_unfactored_matrix": 20.0 * C.nnz + 52.0 * es.n}
        f = db = dx = dC = None
    finally:
        import gc

        gc.collect()
        ctx.close()
    return out


def roofline_3d(args, device):
    """The same two kernels on the 3D Taylor-Hood row pattern of BASELINE config 4 (unit cube, Kuhn tetrahedra, ~90 entries per
    row): SpMV on 24 block-diagonal replicas of C40k (0.9 M rows, 84 M entries, 1.7 GB: beyond the Infinity Cache) and the LU
    sweeps on the factors of one C40k."""
    import lsa_hip
    from synthetic import fem

    es = fem.cube_case("C40k")
    C = sp.csr_matrix((es.A.data - (fem.SIGMA_CUBE + 0.5j) * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    reps, n1, nnz1 = 24, C.shape[0], C.nnz
    rp = np.concatenate([[0], (C.indptr[1:][None, :] + (np.arange(reps) * nnz1)[:, None]).ravel()]).astype(np.int32)
    ci = (C.indices[None, :] + (np.arange(reps, dtype=np.int64) * n1)[:, None]).ravel().astype(np.int32)
    big = sp.csr_matrix((np.tile(C.data, reps), ci, rp), shape=(n1 * reps, n1 * reps))
    ctx = lsa_hip.Context(device)
    try:
        rng = np.random.default_rng(0)
        x = rng.standard_normal(big.shape[0]) + 1j * rng.standard_normal(big.shape[0])
        dB = lsa_hip.CsrMatrix.from_scipy(ctx, big)
        dx = lsa_hip.DeviceVector.from_numpy(ctx, x)
        dy = lsa_hip.DeviceVector(ctx, big.shape[0], np.complex128)
        dB.time_matvec(dx, dy, 5)
        ms = dB.time_matvec(dx, dy, args.roof_iters)
        info = dB.matvec_info(np.complex128)
        bytes_c = 20.0 * big.nnz + 36.0 * big.shape[0]
        out = {"spmv": {"n": big.shape[0], "nnz": int(big.nnz), "kernel": info["kernel"], "ms_per_launch": ms, "algorithmic_bytes": bytes_c,
                        "achieved": bytes_c / ms / 1e6, "frac": bytes_c / ms / 1e6 / HBM_PEAK_GBS, "moved_bytes": info["bytes_moved"]}}
        del dB, dx, dy
        C, tree = ordered_for_lu(C)
        dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
        f = lsa_hip.NdLu(ctx, dC, tree=tree)
        b = rng.standard_normal(n1) + 1j * rng.standard_normal(n1)
        db = lsa_hip.DeviceVector.from_numpy(ctx, b)
        dz = lsa_hip.DeviceVector(ctx, n1, np.complex128)
        f.time_solve(db, dz, 5)
        ms2 = f.time_solve(db, dz, 30)
        li = f.info()
        out["lu_sweeps"] = {"case": "C40k", "n": n1, "ms_per_pair": ms2, "algorithmic_bytes": li["apply_bytes"], "achieved": li["apply_bytes"] / ms2 / 1e6,
                            "frac": li["apply_bytes"] / ms2 / 1e6 / HBM_PEAK_GBS, "max_front": li["max_front"], "levels": li["levels"],
                            "seconds_factor": li["seconds_numeric"], "relative_residual": float(np.linalg.norm(C @ dz.numpy() - b) / np.linalg.norm(b))}
        f = db = dz = dC = None
    finally:
        import gc

        gc.collect()
        ctx.close()
    return out


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir: Path, pairs) -> None:
    """--dump-outputs: what the last timed step returned to its caller, as float64 arrays with a trailing (re, im) axis --
    eigenvalues.npy (k, 2) and eigenvectors.npy (k, n, 2), in the order solve() returned them.  Above 64 MB the
    eigenvectors keep a fixed sample of rows (seed 0, sorted), listed in eigenvector_rows.npy."""
    out_dir.mkdir(parents=True, exist_ok=True)
    lam = np.array([p[0] for p in pairs], dtype=np.complex128)
    vec = np.array([p[1].as_array() for p in pairs], dtype=np.complex128).reshape(len(pairs), -1) if pairs else np.zeros((0, 0), np.complex128)
    split = lambda z: np.stack([z.real, z.imag], axis=-1).astype(np.float64)  # noqa: E731
    np.save(out_dir / "eigenvalues.npy", split(lam))
    k, n = vec.shape
    # (1 MB held back for the eigenvalues and the .npy headers; + 8 bytes per row for the sampled row's index)
    rows_max = (DUMP_BUDGET_BYTES - (1 << 20)) // (16 * k + 8)
    if n > rows_max:
        rows = np.sort(np.random.default_rng(0).choice(n, size=rows_max, replace=False))
        vec = vec[:, rows]
        np.save(out_dir / "eigenvector_rows.npy", rows.astype(np.float64))
    np.save(out_dir / "eigenvectors.npy", split(vec))
    log(f"outputs of the last timed step written to {out_dir}: {k} eigenvalues, eigenvectors {vec.shape[1]} of {n} rows")


def run_sharded_children(args, rank: int, world: int, local_rank: int, case: str | None = None, k: int | None = None, ncv: int | None = None,
                         timeout: float | None = None, port_offset: int = 37, steps: int | None = None):
    """config.sharded at N > 1: every rank starts ONE child process (this file with --sharded-child) that joins a process
    group of its own on another port and solves the sharded problem together with the other ranks' children.  The parent waits
    at most --sharded-timeout seconds and then ends exactly the child it started: whatever the never-exercised multi-rank RCCL
    path does, the parent's bench line survives.  Returns rank 0's record (other ranks: None)."""
    import subprocess

    env = dict(os.environ)
    env.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(local_rank), "MASTER_ADDR": os.environ.get("MASTER_ADDR", "127.0.0.1"),
                "MASTER_PORT": str(int(os.environ.get("MASTER_PORT", "29500")) + port_offset)})
    for var in ("TORCHELASTIC_RUN_ID", "TORCHELASTIC_RESTART_COUNT", "TORCHELASTIC_MAX_RESTARTS", "TORCHELASTIC_USE_AGENT_STORE"):
        env.pop(var, None)  # the child group has its own TCP store (rank 0's child hosts it)
    case = case or args.sharded_case
    limit = args.sharded_timeout if timeout is None else timeout
    cmd = [sys.executable, str(ROOT / "bench.py"), "--sharded-child", "--gpus", str(world), "--steps", str(args.steps if steps is None else steps),
           "--warmup", str(args.warmup), "--case", case, "--k", str(k or args.k), "--ncv", str(ncv or args.ncv), "--atol", str(args.atol), "--no-roofline",
           "--no-cpu-baseline"] + (["--full"] if args.full else [])
    t0 = time.perf_counter()
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        so, se = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        proc.kill()
        so, se = proc.communicate()
        log(f"rank {rank}: the sharded child ({case}) did not finish in {limit:.0f} s and was ended; its last words: {se[-600:]!r}")
        return {"error": f"no result within {limit:.0f} s (child ended by its parent)", "seconds": time.perf_counter() - t0} if rank == 0 else None
    if rank != 0:
        return None
    lines = [ln for ln in so.splitlines() if ln.startswith("{")]
    if proc.returncode != 0 or not lines:
        return {"error": f"child exit code {proc.returncode}: {se[-800:]}", "seconds": time.perf_counter() - t0}
    rec = json.loads(lines[-1])
    cfg = rec.get("config", {})
    keep = {k: cfg.get(k) for k in ("workload", "parallelism", "gmres_iters_per_apply", "allgather_calls_per_solve", "allgather_bytes_received_per_rank_per_solve",
                                    "layout_note", "converged_per_solve", "max_residual", "op_applies_per_solve", "seconds_factor", "setup",
                                    "one_gpu_same_workload_eigenpairs_per_s", "speedup_over_one_gpu_same_workload")}
    keep.update({"eigenpairs_per_s": rec.get("value"), "ms_per_step": rec.get("ms_per_step"), "scaling": rec.get("scaling"), "steps": rec.get("steps"),
                 "seconds": time.perf_counter() - t0,
                 "note": "secondary: ONE problem (BASELINE config 3) row-sharded over the ranks, measured by child processes in a process group of their own"})
    return keep


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", default=None, help="synthetic cylinder case; default S30k on one GPU (BASELINE config 2), S500k for the sharded layout "
                                                 "(BASELINE config 3: the refined mesh row-sharded over the GPUs)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--ncv", type=int, default=80)
    ap.add_argument("--atol", type=float, default=1e-10)
    ap.add_argument("--pc", choices=("lu", "ilu"), default="lu")
    ap.add_argument("--layout", choices=("sharded", "replicas"), default=None,
                    help="N > 1: 'replicas' (default) = the N = 1 workload on every rank, the sharded run as config.sharded; 'sharded' = one problem "
                         "row-sharded over the ranks as the headline")
    ap.add_argument("--sharded-child", action="store_true", help=argparse.SUPPRESS)  # child process of the config.sharded leg
    ap.add_argument("--sharded-timeout", type=float, default=270.0, help="seconds the sharded child processes may take (N > 1)")
    ap.add_argument("--sharded-3d-case", default="C300k", help="N > 1: a second sharded leg on the 3D discretisation (config.sharded_3d; '' = none)")
    ap.add_argument("--sharded-3d-timeout", type=float, default=200.0, help="seconds that leg may take")
    ap.add_argument("--sharded-case", default="S500k")
    ap.add_argument("--sweep", action="store_true", help="replicas layout: one shift of the Re-sweep table per rank instead of N copies of the Re = 50 solve")
    ap.add_argument("--no-other-pc", action="store_true", help="skip the single timed solve of the other inner-solver variant")
    ap.add_argument("--ilu-levels", type=int, default=6, help="fill level of the ILU variant: 2/3/4/6/8/12 -> 14.5/12.2/9.7/8.1/8.2/10.1 s per S30k solve")
    ap.add_argument("--restart", type=int, default=1000)
    ap.add_argument("--roof-case", default="S500k")
    ap.add_argument("--roof-reps", type=int, default=10)
    ap.add_argument("--roof-iters", type=int, default=50)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the other inner-solver variant, solves in flight, LU apply and "
                         "SpTRSV rooflines, the 3D pattern, the SpMV roofline, the CPU baseline (N > 1: the 3D sharded leg and the replicas "
                         "figure). Off: set-up, warm-up, the timed steps and the result line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (eigenvalues, eigenvectors) to DIR/<name>.npy as float64")
    ap.add_argument("--cpu-worker", action="store_true", help=argparse.SUPPRESS)  # child process of the cpu_baseline leg
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_worker:
        args.case = args.case or "S30k"
        _cpu_worker(args)
        return

    # Standard output carries the ONE JSON line and nothing else: whatever a library prints there while the bench runs (gloo's
    # connection banner in a rehearsal, a runtime's notices) is sent to standard error instead.
    sys.stdout.flush()
    line_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        # LSA_BENCH_DEVICE / LSA_BENCH_BACKEND exist only to rehearse the multi-rank code path on a one-GPU box
        # (all ranks on device 0, gloo for the barrier); the driver's runs use one GPU per rank and RCCL.
        dev = int(os.environ.get("LSA_BENCH_DEVICE", local_rank))
        backend = os.environ.get("LSA_BENCH_BACKEND", "nccl")
        torch.cuda.set_device(dev)
        # Five minutes per collective: the longest legitimate wait here is rank 0's roofline legs before the closing barrier
        # (seconds).  A rank that fails on its own while the others sit in a collective then ends the job instead of
        # leaving it to the backend's default of 10-30 minutes.
        from datetime import timedelta

        # (a child lives at most --sharded-timeout seconds; the parents wait for their children inside barriers of THEIR group)
        pg_timeout = timedelta(seconds=120 if args.sharded_child else max(600.0, 2.0 * (args.sharded_timeout + args.sharded_3d_timeout) + 120.0))
        if backend == "nccl":
            dist_mod.init_process_group("nccl", device_id=torch.device("cuda", dev), timeout=pg_timeout)
        else:
            dist_mod.init_process_group(backend, timeout=pg_timeout)
        dist = dist_mod
        reduce_device = "cuda" if backend == "nccl" else "cpu"
    device = int(os.environ.get("LSA_BENCH_DEVICE", local_rank)) if world > 1 else 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an AMD GPU (no CPU fallback)")
    # PyTorch's own lazy device initialisation happens HERE, before anything is built or warmed up: left to the first
    # barrier() it landed between the warm-up and the timed steps, and the first timed solve then took 100 instead of 73 ms
    torch.cuda.set_device(device)
    torch.cuda.synchronize()

    from synthetic import fem

    layout = "single" if world == 1 else ("sharded" if args.sharded_child else (args.layout or "replicas"))
    if args.sweep:
        layout = "replicas"
    sharded = layout == "sharded"
    if args.case is None:
        args.case = args.sharded_case if sharded else "S30k"
    cube = args.case.startswith("C")  # the 3D discretisation of BASELINE config 4 (the second sharded leg of an N > 1 run)
    es = fem.cube_case(args.case) if cube else fem.cylinder_case(args.case)
    sigma = complex(fem.SIGMA_CUBE) if cube else SWEEP_SIGMAS[(2 + rank) % len(SWEEP_SIGMAS)] if args.sweep else SWEEP_SIGMAS[2]
    log(f"rank {rank}/{world}: {args.case} n={es.n} nnz={es.A.nnz} sigma={sigma} layout={layout}")

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    layout_note = None
    solver = None
    setup = {}
    if sharded:
        # The sharded layout has more moving parts than anything else here (forest cut, RCCL bootstrap, exchange regions): if
        # setting it up or the first solve fails on EVERY rank (a deterministic failure), the ranks fall back to independent
        # replicas and the line says so -- a bench line with a note instead of no line.  (The ranks agree through the
        # launcher's process group; a failure on SOME ranks only leaves the others inside the setup's own collectives and
        # ends with the process group's time-out, as it would without this.)
        ok, why = 1, ""
        try:
            if os.environ.get("LSA_BENCH_FAIL_SHARDED") in (str(rank), "all"):  # development: rehearse the fall-back below
                raise RuntimeError("forced failure of the sharded setup (LSA_BENCH_FAIL_SHARDED)")
            solver = build_solver(es, sigma, args, device, args.pc, "sharded")
            solver.solver.prepare()
            # The stream-ordered exchange inside batched Arnoldi steps has never run with more than one rank on hardware the
            # build could reach: the first solve reads every step back (LSA_KRYLOV_BATCH=1), the second runs the batched
            # steps, and their eigenvalues must agree before anything is timed.
            os.environ["LSA_KRYLOV_BATCH"] = "1"
            try:
                solver.solve()
            finally:  # (left set after a failure, everything after it in this process would read every step back)
                os.environ.pop("LSA_KRYLOV_BATCH", None)
            lam_one = np.array([solver.solver.get_eigenvalue(i) for i in range(solver.solver.get_num_converged())])
            solver.solve()
            lam_bat = np.array([solver.solver.get_eigenvalue(i) for i in range(solver.solver.get_num_converged())])
            kk = min(len(lam_one), len(lam_bat), args.k)
            batch_gap = float(np.max(np.abs(lam_one[:kk] - lam_bat[:kk]) / np.abs(lam_one[:kk]))) if kk else float("inf")
            if not (kk >= args.k and batch_gap <= 1e-9):
                raise RuntimeError(f"batched Arnoldi steps disagree with one step at a time over {world} ranks: {kk} common pairs, gap {batch_gap:.2e}")
            setup["batched_vs_stepwise_max_rel_gap"] = batch_gap
        except Exception as exc:  # noqa: BLE001
            ok, why = 0, f"{type(exc).__name__}: {exc}"
            log(f"rank {rank}: sharded layout failed: {why}")
        flag = torch.tensor([ok], dtype=torch.int32, device=reduce_device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            layout_note = "sharded layout failed on at least one rank (" + (why or "another rank") + "): independent replicas of the same problem instead"
            if solver is not None:
                try:
                    solver.solver.release()
                except Exception:  # noqa: BLE001
                    pass
            solver, sharded, layout = None, False, "replicas"
    if solver is None:
        solver = build_solver(es, sigma, args, device, args.pc, "single")
        t_p = time.perf_counter()
        solver.solver.prepare()  # ordering + upload + pattern analysis: (A, M) now resident in HBM
        setup["prepare_ms"] = 1e3 * (time.perf_counter() - t_p)
        solver.solve()
        setup["cold_first_solve_ms"] = 1e3 * (time.perf_counter() - t_p)  # what a caller with one eigenproblem pays, kernel loading included
        setup["first_solve_ms"] = setup["cold_first_solve_ms"] - setup["prepare_ms"]
    # Set-up ends with the process's first TWO solves (the sharded branch above has done one): under PyTorch's bundled ROCm
    # runtime the second solve of a process takes 100-113 ms instead of 73 -- 26-39 ms inside one stream synchronisation
    # after the Ritz-vector product, once, and not with /opt/rocm's runtime (tools/micro/first_solves.py) -- a one-time cost
    # of the runtime like the first solve's kernel loading, not of a step.  The W warm-up steps and the K timed steps follow.
    solver.solve()
    for _ in range(args.warmup):
        solver.solve()
    barrier()
    t0 = time.perf_counter()
    step_marks = [t0]
    for _ in range(args.steps):
        last_pairs = solver.solve()
        step_marks.append(time.perf_counter())
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(Path(args.dump_outputs), last_pairs)
    log("seconds per step: " + " ".join(f"{b - a:.3f}" for a, b in zip(step_marks[:-1], step_marks[1:]))
        + f"; last solve: factor {solver.solver.stats.get('seconds_factor', 0.0):.3f} s, Arnoldi {solver.solver.stats.get('seconds_solve', 0.0):.3f} s")
    # count pairs that pass the true residual test (device evaluation, after the timed region)
    res = solver.solver.residuals()
    nconv = int(np.sum(res[: args.k] <= RESIDUAL_TOL))
    stats = solver.solver.stats
    total_pairs = float(nconv * args.steps)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=reduce_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if not sharded:  # replicas: every rank solved a problem of its own; sharded: the ranks solved ONE problem together
            p = torch.tensor([total_pairs], dtype=torch.float64, device=reduce_device)
            dist.all_reduce(p, op=dist.ReduceOp.SUM)
            total_pairs = float(p.item())
    lam_gpu = np.array([solver.solver.get_eigenvalue(i) for i in range(min(args.k, solver.solver.get_num_converged()))])
    solver.solver.release()
    sharded_rec = sharded_3d = None
    if world > 1 and not sharded and not args.sharded_child and not args.no_other_pc and args.sharded_timeout > 0:
        barrier()  # every parent has released its solver: the children find the GPUs free
        sharded_rec = run_sharded_children(args, rank, world, local_rank)
        barrier()
        if args.full and args.sharded_3d_case and args.sharded_3d_timeout > 0:
            # BASELINE config 4's discretisation over the ranks, top fronts of the forest distributed: informative only
            sharded_3d = run_sharded_children(args, rank, world, local_rank, case=args.sharded_3d_case, k=10, ncv=40, timeout=args.sharded_3d_timeout,
                                              port_offset=53, steps=min(args.steps, 3))
            barrier()
    replicas = None
    if args.full and sharded and not args.no_other_pc:
        # secondary figure: the same N GPUs as N independent solves of the N = 1 workload (no data-path collective)
        try:
            so = build_solver(es, sigma, args, device, args.pc)
            so.solver.prepare()
            so.solve()
            barrier()
            t1 = time.perf_counter()
            for _ in range(2):
                so.solve()
            barrier()
            dt = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=reduce_device)
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
            nrep = torch.tensor([2.0 * int(np.sum(so.solver.residuals()[: args.k] <= RESIDUAL_TOL))], dtype=torch.float64, device=reduce_device)
            dist.all_reduce(nrep, op=dist.ReduceOp.SUM)
            replicas = {"eigenpairs_per_s": float(nrep.item()) / float(dt.item()), "ms_per_step": 1e3 * float(dt.item()) / 2, "scaling": "weak",
                        "note": f"secondary: every rank solves the same {args.case} problem on its own GPU at the same time (no data-path collective); "
                                "eigenpairs_per_s / n_gpus is the one-GPU rate of this workload, the reference point of the sharded run's strong scaling"}
            so.solver.release()
        except Exception as exc:  # noqa: BLE001  (every rank takes the same path: the collectives above stay matched)
            replicas = {"error": f"{type(exc).__name__}: {exc}"}
    other = None
    if args.full and rank == 0 and not args.no_other_pc and world == 1 and not args.sharded_child:
        opc = "ilu" if args.pc == "lu" else "lu"
        try:  # the other inner-solver variant is informative only: it must never cost the bench line
            so = build_solver(es, sigma, args, device, opc)
            so.solver.prepare()
            t1 = time.perf_counter()
            so.solve()
            dt = time.perf_counter() - t1
            ro = so.solver.residuals()
            no = int(np.sum(ro[: args.k] <= RESIDUAL_TOL))
            sto = so.solver.stats
            other = {"pc": f"ilu({args.ilu_levels})-gmres" if opc == "ilu" else "lu", "ilu_fill_level": args.ilu_levels if opc == "ilu" else None,
                     "eigenpairs_per_s": no / dt, "seconds_per_solve": dt, "converged": no, "op_applies": sto.get("op_applies"),
                     "gmres_iters": sto.get("gmres_iters"), "seconds_factor": sto.get("seconds_factor")}
            so.solver.release()
        except Exception as exc:  # noqa: BLE001
            other = {"pc": opc, "error": f"{type(exc).__name__}: {exc}"}

    if rank == 0:
        out = {
            "metric": "converged eigenpairs/sec (k=20, shift-invert)",
            "value": total_pairs / elapsed,
            "unit": "eigenpairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "strong" if sharded else "weak",
            "vs_baseline": None,
            "dtype": "c128",
            "data": "synthetic",
            "config": {
                "workload": f"{args.case}: synthetic " + ("3D unit-cube duct Taylor-Hood pair (BASELINE config 4's discretisation)" if cube else "2D cylinder-flow Taylor-Hood pair")
                            + f", n={es.n}, nnz={es.A.nnz}, Re={10 if cube else 50}, "
                            f"sigma={sigma.real:g}{sigma.imag:+g}j, k={args.k}, ncv={args.ncv}, outer tol {args.atol:g}, "
                            + ("inner solves: exact nested-dissection multifrontal LU (verified against b - C x, GMRES-wrapped)" if args.pc == "lu"
                               else f"inner solves: ILU({args.ilu_levels})-GMRES({args.restart}), blocked SpTRSV"),
                "pc": args.pc,
                "other_pc": other,
                "layout": "single GPU" if world == 1 else "sharded" if sharded else "replicas: one shift of the Re sweep per rank" if args.sweep
                          else f"replicas: every rank solves the same {args.case} problem (fall-back from the sharded layout)" if layout_note
                          else "replicas of the N = 1 workload",
                "parallelism": None if world == 1 else (
                    (f"one problem over {world} ranks, Krylov bases replicated, "
                     + ("subtree-parallel exact LU (own subtrees of the nested-dissection forest, all-gather of the subtree roots' update "
                        "vectors, replicated top, all-gather of the solution); the sparse products replicated on the 2D pattern, "
                        "on the rank's rows + all-gather on the 3D one" if args.pc == "lu"
                        else "rows of A, M, C sharded, block-Jacobi ILU(k) + GMRES, all-gather after every SpMV and preconditioner apply")) if sharded
                    else f"{world} independent solves"),
                "gmres_iters_per_apply": (stats.get("gmres_iters", 0) / max(stats.get("op_applies", 1), 1)) if sharded else None,
                "allgather_calls_per_solve": stats.get("allgather_calls") if sharded else None,
                "allgather_bytes_received_per_rank_per_solve": stats.get("allgather_bytes_received") if sharded else None,
                "layout_note": layout_note,
                "replicas": replicas,
                "one_gpu_same_workload_eigenpairs_per_s": (replicas["eigenpairs_per_s"] / world) if (sharded and replicas and "eigenpairs_per_s" in replicas) else None,
                "speedup_over_one_gpu_same_workload": (total_pairs / elapsed) / (replicas["eigenpairs_per_s"] / world)
                if (sharded and replicas and "eigenpairs_per_s" in replicas) else None,
                "sharded": sharded_rec,
                "sharded_3d": sharded_3d,
                "setup": setup,
                "prepare_ms": setup.get("prepare_ms"),
                "cold_first_solve_ms": setup.get("cold_first_solve_ms"),
                "setup_solves": 2,
                "converged_per_solve": nconv,
                "max_residual": float(res[: args.k].max()) if len(res) else None,
                "op_applies_per_solve": stats.get("op_applies"),
                "gmres_iters_per_solve": stats.get("gmres_iters"),
                "seconds_factor": stats.get("seconds_factor"),
                # phases of the last timed solve inside the library's Krylov-Schur loop: Arnoldi steps (GPU), the host's dense
                # algebra on the projected matrix (Schur forms, reordering), basis updates and Ritz vectors (GPU)
                "seconds_expand": stats.get("seconds_expand"),
                "seconds_dense": stats.get("seconds_dense"),
                "seconds_restart": stats.get("seconds_restart"),
            },
        }
        if args.full and world == 1 and not args.no_other_pc:
            for name, fn in (("two_solves_in_flight", lambda: solves_in_flight(es, sigma, args, device)),
                             # (three is the most one GPU takes: with four the solves' streams outnumber the hardware queues and
                             #  the rate falls below that of two -- tools/micro/jobs_in_flight.py: 385 / 589 / 756 / 483 at J = 1..4)
                             ("three_solves_in_flight", lambda: solves_in_flight(es, sigma, args, device, jobs=3)),
                             ("lu_apply", lambda: lu_apply_rate(es, sigma, device)),
                             ("sptrsv_roofline", lambda: sptrsv_roofline(args, device)),
                             ("pattern_3d", lambda: roofline_3d(args, device))):
                try:  # secondary figures must never cost the bench line
                    out["config"][name] = fn()
                except Exception as exc:  # noqa: BLE001
                    out["config"][name] = {"error": f"{type(exc).__name__}: {exc}"}
        la = out["config"].get("lu_apply")
        out["config"]["analysis_ms"] = 1e3 * la["seconds_analyse"] if isinstance(la, dict) and "seconds_analyse" in la else None
        if args.full and not args.no_roofline:
            try:
                roof = spmv_roofline(args, device)
                out["roofline"] = {
                    "bound": "hbm", "achieved": roof["c128"]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": roof["c128"]["gbs"] / HBM_PEAK_GBS, "traffic": pmc_traffic(args, roof["c128"]["kernel"]),
                    "kernel": roof["c128"]["kernel"] + " on SROOF", "ms_per_launch": roof["c128"]["ms"],
                    "algorithmic_bytes_per_launch": roof["c128"]["bytes"],
                    # the kernel's own byte count (2-byte column offsets when the compressed form runs): what it really streams
                    "moved_bytes_per_launch": roof["c128"]["moved"], "achieved_moved": roof["c128"]["moved_gbs"],
                    "frac_moved": roof["c128"]["moved_gbs"] / HBM_PEAK_GBS, "n": roof["n"], "nnz": roof["nnz"],
                    "f64": {"achieved": roof["f64"]["gbs"], "frac": roof["f64"]["gbs"] / HBM_PEAK_GBS, "ms_per_launch": roof["f64"]["ms"],
                            "kernel": roof["f64"]["kernel"]},
                }
            except Exception as exc:  # noqa: BLE001  (the headline value must survive a failure of this leg)
                out["roofline"] = {"error": f"{type(exc).__name__}: {exc}"}
        if world > 1:
            # the CPU baseline is a leg of the N = 1 run (same S30k workload as its GPU line); the sharded run's workload
            # takes the oracle many minutes and would hold the other ranks in the closing barrier
            out["cpu_baseline"] = None
        elif args.full and not args.no_cpu_baseline:
            try:
                base, lam_cpu = cpu_baseline(es, sigma, args)
                out["cpu_baseline"] = base
                if len(lam_gpu):
                    out["config"]["max_rel_eig_diff_vs_cpu"] = float(max(np.min(np.abs(lam_gpu - r)) / abs(r) for r in lam_cpu[: len(lam_gpu)]))
                opc_rec = out["config"].get("other_pc")
                if isinstance(opc_rec, dict) and "eigenpairs_per_s" in opc_rec and str(opc_rec.get("pc", "")).startswith("ilu"):
                    # ILU(k)-GMRES is the memory-lean alternative, kept for problems whose exact factors do not fit; where they do
                    # fit it does not compete: said on the line, with the fill level it was run at (ILU(0), the north star's
                    # wording, does not converge at this size: tests/test_gpu_eigen.py covers it where it does)
                    opc_rec["status"] = ("not competitive: slower than the one-core CPU baseline" if opc_rec["eigenpairs_per_s"] < base["value"]
                                         else "slower than the exact LU by %.0fx" % (out["value"] / max(opc_rec["eigenpairs_per_s"], 1e-300)))
            except Exception as exc:  # noqa: BLE001
                out["cpu_baseline"] = {"error": f"{type(exc).__name__}: {exc}"}
        if world > 1 and not sharded and isinstance(sharded_rec, dict) and "error" not in sharded_rec and sharded_rec.get("eigenpairs_per_s") \
                and not sharded_rec.get("layout_note") and (sharded_rec.get("converged_per_solve") or 0) >= args.k:
            # The layout BASELINE.json names for N > 1 is the headline once it has passed its own checks in this run (batched
            # against stepwise Arnoldi steps, k converged pairs on their true residuals): ONE problem (config 3) over all ranks,
            # strong scaling.  The replicas of the N = 1 workload measured above stay on the line as config.replicas.
            out["config"]["replicas"] = {"eigenpairs_per_s": out["value"], "ms_per_step": out["ms_per_step"], "scaling": "weak",
                                         "workload": out["config"]["workload"],
                                         "note": f"every rank solves the {args.case} problem of the N = 1 line on its own GPU (no data-path collective)"}
            out["value"] = sharded_rec["eigenpairs_per_s"]
            out["ms_per_step"] = sharded_rec["ms_per_step"]
            out["scaling"] = "strong"
            out["config"]["workload"] = sharded_rec.get("workload")
            out["config"]["layout"] = "sharded"
            out["config"]["parallelism"] = sharded_rec.get("parallelism")
            out["config"]["layout_note"] = (f"value = the sharded run of {args.sharded_case} over {world} ranks (config.sharded, measured by child processes "
                                            "after its batched-vs-stepwise check passed); config.replicas = the N = 1 workload on every rank; "
                                            "config.sharded.one_gpu_same_workload_eigenpairs_per_s is the one-GPU rate of the value's workload")
        elif world > 1 and not sharded and not args.sharded_child:
            out["config"]["layout_note"] = ((layout_note + "; ") if layout_note else "") + \
                "value = independent replicas of the N = 1 workload, weak scaling WITHOUT communication: the sharded run did not produce a checked result (" + \
                (str(sharded_rec.get("error") or sharded_rec.get("layout_note"))[:300] if isinstance(sharded_rec, dict) else "not run") + ")"
            out["sharded_failed"] = True
        os.write(line_fd, (json.dumps(out) + "\n").encode())
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
