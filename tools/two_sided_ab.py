"""Left and right eigenvectors: one two-sided solve against the two separate solves it replaces.

    python tools/two_sided_ab.py [--cases S30k C160k] [--reps 3] [--out profiles/two_sided_ab.json]

``separate``: a fresh direct solver at sigma, then a fresh ``adjoint=True`` solver at conj(sigma) -- two set-ups, two factorisations,
two iterations (what ``Sensitivity.solve_direct_mode`` + ``solve_adjoint_mode`` cost, apart from where the second one shifts).
``two_sided``: one fresh ``two_sided=True`` solver -- one set-up, one factorisation, the direct iteration, the adjoint iteration on
the same factors and basis, the pairing.  S30k in the bench configuration (k = 20, ncv = 80, tol 1e-10, sigma = SIGMA_RE50) and the
3D case C160k at k = 10 (ncv = 40, sigma = SIGMA_CUBE).  Every timed sample builds its solvers anew (construction, ``prepare``,
``solve``, ``release`` inside the clock); the two settings alternate in one process after one warm-up of each; medians and spread
over ``reps`` samples, with the phase split of the library's clocks.  No test asserts these times.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

SPLIT = ("seconds_factor", "seconds_expand", "seconds_dense", "seconds_restart")
CASES = {"S30k": {"k": 20, "ncv": 80}, "C160k": {"k": 10, "ncv": 40}}


def problem(case: str):
    from synthetic import fem

    if case.startswith("C"):
        return fem.cube_case(case), fem.SIGMA_CUBE
    return fem.cylinder_case(case), fem.SIGMA_RE50


def fresh(es, sigma, k: int, ncv: int, **kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=k, atol=1e-10, ncv=ncv, max_it=500), check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(sigma)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def timed(es, sigma, k, ncv, **kw) -> dict:
    """One fresh solver from construction to release; the seconds outside the library's clocks are set-up and host work."""
    t0 = time.perf_counter()
    s = fresh(es, sigma, k, ncv, **kw)
    s.solver.prepare()
    t1 = time.perf_counter()
    pairs = s.solve()
    t2 = time.perf_counter()
    st = s.solver.stats
    s.solver.release()
    lam = np.array([p[0] for p in pairs], dtype=np.complex128)
    out = {"eigenvalues": lam, "seconds": time.perf_counter() - t0, "seconds_prepare": t1 - t0, "seconds_solve_call": t2 - t1, "pairs": len(pairs),
           "applies": st["op_applies"], "restarts": st["krylov_restarts"], **{name: st.get(name, 0.0) for name in SPLIT}}
    if "left" in st:
        left = st["left"]
        out["left"] = {name: left[name] for name in ("applies", "restarts", "seconds", "seconds_solve", "refactored", "unmatched", "biorth_defect")}
        kappa = s.solver.get_condition_numbers()
        out["kappa_max"] = float(np.nanmax(kappa)) if kappa.size else 0.0
    return out


def sample(es, sigma, k, ncv, two_sided: bool) -> dict:
    if two_sided:
        return timed(es, sigma, k, ncv, two_sided=True)
    direct = timed(es, sigma, k, ncv)
    adjoint = timed(es, np.conj(sigma), k, ncv, adjoint=True)
    return {"seconds": direct["seconds"] + adjoint["seconds"], "eigenvalues": direct["eigenvalues"], "adjoint_eigenvalues": adjoint["eigenvalues"],
            "direct": direct, "adjoint": adjoint}


def same_answer(separate: dict, two_sided: dict) -> float:
    """Before anything is timed: both routes return the same eigenvalues (the two-sided solve's direct phase is the plain solve), and
    the separate adjoint solve's are their conjugates; the largest relative difference of the latter."""
    lam, lam2, mu = separate["eigenvalues"], two_sided["eigenvalues"], separate["adjoint_eigenvalues"]
    if lam.shape != lam2.shape or not np.array_equal(lam, lam2):
        raise SystemExit(f"the two routes return different eigenvalues: {lam} against {lam2}")
    worst = max(float(np.min(np.abs(np.conj(mu) - z)) / abs(z)) for z in lam)
    if worst > 1e-6:
        raise SystemExit(f"the separate adjoint solve found other eigenvalues (relative distance {worst:.2e}): {mu} against conj of {lam}")
    return worst


def plain(run: dict) -> dict:
    """A sample without its arrays (JSON)."""
    return {k: (plain(v) if isinstance(v, dict) else v) for k, v in run.items() if not isinstance(v, np.ndarray)}


def spread(values) -> dict:
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "two_sided_ab.json")
    args = ap.parse_args(argv)
    result = {"config": {"tol": 1e-10, "reps": args.reps, "cases": {c: CASES[c] for c in args.cases}}, "cases": []}
    for case in args.cases:
        es, sigma = problem(case)
        k, ncv = CASES[case]["k"], CASES[case]["ncv"]
        runs = {False: [], True: []}
        warm = {flag: sample(es, sigma, k, ncv, flag) for flag in (False, True)}  # warm-up: code objects, buffers
        adjoint_difference = same_answer(warm[False], warm[True])
        for _ in range(args.reps):
            for flag in (False, True):
                runs[flag].append(sample(es, sigma, k, ncv, flag))
        entry = {"case": case, "n": int(es.A.shape[0]), "k": k, "ncv": ncv, "sigma": [complex(sigma).real, complex(sigma).imag],
                 "separate": {"seconds": spread([r["seconds"] for r in runs[False]]),
                              "direct_seconds": spread([r["direct"]["seconds"] for r in runs[False]]),
                              "adjoint_seconds": spread([r["adjoint"]["seconds"] for r in runs[False]]), "last": plain(runs[False][-1])},
                 "two_sided": {"seconds": spread([r["seconds"] for r in runs[True]]),
                               "left_seconds": spread([r["left"]["seconds"] for r in runs[True]]), "last": plain(runs[True][-1])},
                 "eigenvalues_equal": True, "adjoint_eigenvalue_difference": adjoint_difference}
        entry["speedup_median"] = entry["separate"]["seconds"]["median"] / entry["two_sided"]["seconds"]["median"]
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
