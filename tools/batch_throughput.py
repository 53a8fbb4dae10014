"""Throughput of a Reynolds sweep on the bench case: Solver.eigen.solve_batch, in turn and in lockstep, against a solo loop and three
solves in flight.

    python tools/batch_throughput.py [--case S30k] [--sizes 1 2 4 8] [--reps 2] [--out profiles/batch_throughput.json]

J Reynolds numbers of ``synthetic.fem.cylinder_case(case, re)`` with the harness's tabulated targets
(``lsa-fw_amd/examples/eigenvalues.py``), the bench configuration (k = 20, ncv = 80, tol 1e-10, shift-invert, exact LU).
Each mode builds fresh solvers, solves all J problems and releases them; set-up (ordering, analysis, uploads) counts,
as it does in the harness.  Modes alternate inside one process, ``reps`` times per J:

- ``solo``: one problem after another, each with its own context, ordering and analysis;
- ``batch``: ``solve_batch(max_batch=J)``: one context, ordering and analysis per group, the problems one after another;
- ``lockstep``: ``solve_batch(max_batch=J, lockstep=True)``: all J factorisations first, then one ``lsa_krylov_solve_batch`` whose
  Arnoldi rounds hold one step of every problem (batched sweeps, batched DCGS2 launches); also reports the rounds, the launches
  per round and the read-backs of the group's call;
- ``threads3``: three solo solves in flight (threads, one context each: ``examples/eigenvalues.py --jobs 3``).

Per mode: aggregate eigenpairs/s (median over reps) and the time split from the solvers' statistics -- numeric
factorisations, Arnoldi expansion (device steps), host dense work (Schur forms), restarts and Ritz vectors, and the rest
(ordering, analysis, uploads, Python), in total and per problem.  Under lockstep the expansion time of a problem is its share
(1 / active problems) of the wall time of the group's expansions, and the dense phase of the J problems runs back to back on
the host with the device idle: its share of the wall time is reported.  Every batched problem is checked bit for bit against
its solo solve.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j), (0.03 + 0.742986662573986j),
           (0.05 + 0.744243299635422j), (0.061 + 0.7461282552275759j), (0.072 + 0.7461282552275759j), (0.085 + 0.744557458900781j),
           (0.09 + 0.742986662573986j), (0.1 + 0.7398450699203962j), (0.115 + 0.7351326809400116j))
REYNOLDS = tuple(range(40, 91, 5))
SPLIT = ("seconds_factor", "seconds_expand", "seconds_dense", "seconds_restart")


def build(es, target):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=20, atol=1e-10, ncv=80, max_it=500), check_hermitian=False)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(target)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def outcome(s, pairs):
    st = s.solver.stats
    return {"pairs": len(pairs), "lam": s.solver._eigenvalues.copy(), "X": np.array(s.solver._eigenvectors), **{k: st.get(k, 0.0) for k in SPLIT},
            **{k: st[k] for k in ("lockstep_steps", "solo_steps", "lockstep_rounds", "lockstep_launches_per_round") if k in st}}


def run_solo(problems):
    out = []
    for es, target in problems:
        s = build(es, target)
        out.append(outcome(s, s.solve()))
        s.solver.release()
    return out


def run_batch(problems, lockstep=False):
    from Solver.eigen import solve_batch

    solvers = [build(es, target) for es, target in problems]
    pairs = solve_batch(solvers, max_batch=len(solvers), lockstep=lockstep)
    out = [outcome(s, p) for s, p in zip(solvers, pairs)]
    for s in solvers:
        s.solver.release()
    return out


def run_threads(problems, pool):
    def one(es, target):
        s = build(es, target)
        r = outcome(s, s.solve())
        s.solver.release()
        return r

    return [f.result() for f in [pool.submit(one, es, target) for es, target in problems]]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S30k")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "batch_throughput.json")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # three solves in flight (examples/eigenvalues.py --jobs)
    os.environ.setdefault("LSA_HOST_BLAS_THREADS", "1")
    from synthetic import fem

    jmax = max(args.sizes)
    t0 = time.time()
    cases = [(fem.cylinder_case(args.case, re=float(REYNOLDS[i])), TARGETS[i]) for i in range(jmax)]
    print(f"{jmax} x {args.case} assembled in {time.time() - t0:.1f} s (n = {cases[0][0].A.shape[0]})", flush=True)
    run_solo(cases[:1])  # kernel loading and first-context costs outside the timings
    rows = []
    bitwise = True
    with ThreadPoolExecutor(max_workers=3) as pool:
        run_threads(cases[:3], pool)
        for J in args.sizes:
            problems = cases[:J]
            rec = {"J": J}
            samples = {m: [] for m in ("solo", "batch", "lockstep", "threads3")}
            splits = {m: None for m in samples}
            for _ in range(args.reps):
                for mode in samples:
                    t = time.perf_counter()
                    res = (run_solo(problems) if mode == "solo" else run_batch(problems) if mode == "batch"
                           else run_batch(problems, lockstep=True) if mode == "lockstep" else run_threads(problems, pool))
                    wall = time.perf_counter() - t
                    samples[mode].append(sum(r["pairs"] for r in res) / wall)
                    split = {k: sum(r[k] for r in res) for k in SPLIT}
                    split["seconds_other"] = wall - sum(split.values()) if mode != "threads3" else None
                    split["seconds_wall"] = wall
                    split["per_problem_ms"] = {k[len("seconds_"):]: 1e3 * split[k] / J for k in SPLIT}
                    split["dense_share_of_wall"] = split["seconds_dense"] / wall
                    if mode == "lockstep":
                        split.update({"rounds": res[0].get("lockstep_rounds", 0), "launches_per_round": res[0].get("lockstep_launches_per_round", 0.0),
                                      "lockstep_steps": [r.get("lockstep_steps", 0) for r in res], "solo_steps": [r.get("solo_steps", 0) for r in res]})
                    splits[mode] = split
                    if mode == "solo":
                        solo = res
                    if mode in ("batch", "lockstep"):
                        same = all(np.array_equal(b["lam"], s["lam"]) and np.array_equal(b["X"], s["X"]) for b, s in zip(res, solo))
                        bitwise &= same
            for mode, v in samples.items():
                rec[f"{mode}_eigenpairs_per_s"] = statistics.median(v)
                rec[f"{mode}_samples"] = v
                rec[f"{mode}_split_last"] = splits[mode]
            rec["batch_over_solo"] = rec["batch_eigenpairs_per_s"] / rec["solo_eigenpairs_per_s"]
            rec["batch_over_threads3"] = rec["batch_eigenpairs_per_s"] / rec["threads3_eigenpairs_per_s"]
            rec["lockstep_over_batch"] = rec["lockstep_eigenpairs_per_s"] / rec["batch_eigenpairs_per_s"]
            rec["lockstep_over_threads3"] = rec["lockstep_eigenpairs_per_s"] / rec["threads3_eigenpairs_per_s"]
            rec["expand_ms_per_problem"] = {m: splits[m]["per_problem_ms"]["expand"] for m in ("solo", "batch", "lockstep")}
            rows.append(rec)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith(("_samples", "_split_last"))}), flush=True)
    out = {"case": args.case, "config": "k=20, ncv=80, tol=1e-10, SINVERT, exact LU", "reps": args.reps,
           "batch_bit_identical_to_solo": bool(bitwise), "rows": rows}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(out, indent=1) + "\n")
    print(f"batched problems bit-identical to solo solves: {bitwise}; written {args.out}")
    if not bitwise:
        sys.exit(1)


if __name__ == "__main__":
    main()
