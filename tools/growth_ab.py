"""Optimal transient growth: the library's iteration against what a user can drive from the host on kept factors.

    python tools/growth_ab.py [--cases S30k C160k] [--reps 3] [--scheme euler] [--windows] [--out profiles/growth_ab.json]

``library`` (a): ``Solver.growth.TransientGrowthSolver.solve`` -- set-up, one factorisation of ``A - M / dt``, the thick-restart Lanczos
iteration on ``W = Phi+ Phi`` with the march of ``2 N`` solves, its checks, the mask and the orthogonalisation on the device, one
read-back per step.
``host`` (b): ``scipy.sparse.linalg.eigsh`` on a ``LinearOperator`` whose product marches through ``iKSP`` on ONE kept factorisation of
the same matrix (``N`` calls of ``solve``, ``N`` of ``solve_many(adjoint=True)``), the products with ``M`` and the mask in scipy: ``2 N``
host round trips per product.  ``W`` is self-adjoint in the ``M``-inner product, not in the Euclidean one, and ``M`` is singular (zero
pressure block), so (b) solves the equivalent symmetric-definite problem ``S y = theta M_uu y`` on the dofs ``u`` that carry mass and are
free, ``S = (Phi^T M Phi)_uu`` (``Phi = Xi M`` never sees the other dofs of its argument), with SuperLU for ``M_uu``.

dt 0.25, T = 4 (N = 16), num_modes 2, ncv 12, tolerance 1e-8.  Every timed sample builds its solver anew (construction, preparation,
factorisation, iteration, release inside the clock); the two settings alternate in one process after one warm-up of each; medians
and spread over ``reps`` samples.  The gains of (b) are compared with those of (a).  No test asserts these times.

``--scheme sdirk2``: both settings take the two-stage step ``S (a S + b I)`` on the factorisation of ``A - M / (gamma dt)`` (``4 N`` solves
per product; (b): ``4 N`` round trips).  Its results go under the key ``"sdirk2"`` of the output file, beside the Euler rows.

``--windows`` compares the library's solve with a response window (x in [2, 30]; cylinder cases) against its plain solve and against
the plain problem solved through a window of ones (the same iteration with a windowed copy of ``M`` at the turn), alternately
after a warm-up of each; the result goes under the key ``growth`` of ``profiles/windows_ab.json``.  Only the turn of a step's march
differs, so the figure to compare is ``seconds_per_step``.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

DT, HORIZON, MODES, NCV, TOL = 0.25, 4.0, 2, 12, 1e-8
SCHEME = "euler"  # (main sets it from --scheme)
SDIRK_A, SDIRK_B = 1.0 + np.sqrt(2.0), -np.sqrt(2.0)


def problem(case: str):
    from synthetic import fem

    return fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)


RESPONSE_STRIP = (2.0, 30.0)


def response_window(es) -> np.ndarray:
    """The 0/1 response window of a cylinder case."""
    x, _ = es.dof_xy()
    return ((x >= RESPONSE_STRIP[0]) & (x <= RESPONSE_STRIP[1])).astype(float)


def library(es, windows=False) -> dict:
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    t0 = time.perf_counter()
    tg = TransientGrowthSolver(es.A, es.M, TransientGrowthConfig(dt=DT, num_modes=MODES, ncv=NCV, atol=TOL, scheme=SCHEME),
                               response_window=np.ones(es.n) if windows == "ones" else response_window(es) if windows else None)
    tg.solver.prepare()
    t1 = time.perf_counter()
    res = tg.solve(HORIZON)
    t2 = time.perf_counter()
    tg.release()
    st = res.stats
    steps = max(st["applies"], 1)
    return {"gains": res.gains, "seconds": time.perf_counter() - t0, "seconds_setup": t1 - t0, "seconds_solve_call": t2 - t1,
            "seconds_factor": st["seconds_factor"], "seconds_steps": st["seconds_expand"], "seconds_host_dense": st["seconds_dense"],
            "seconds_restart": st["seconds_restart"], "applies": st["applies"], "restarts": st["restarts"], "refinements": st["refinements"],
            "forward_solves": st["forward_solves"], "transposed_solves": st["transposed_solves"], "constrained": st["constrained"],
            "seconds_per_step": st["seconds_expand"] / steps, "read_backs_per_step": 1}


def host(es) -> dict:
    from Solver.growth import SCHEMES, decoupled_dofs
    from Solver.utils import KSPType, PreconditionerType, iKSP

    t0 = time.perf_counter()
    A, M = sp.csr_matrix(es.A), sp.csr_matrix(es.M)
    n, sigma, steps = A.shape[0], 1.0 / (SCHEMES[SCHEME] * DT), round(HORIZON / DT)
    two = SCHEME == "sdirk2"
    keep = np.ones(n)
    keep[decoupled_dofs(A, M)] = 0.0
    u = np.flatnonzero((keep == 1.0) & (M.diagonal() > 0.0))  # free dofs that carry mass
    Muu = M[u][:, u].tocsc()
    ksp = iKSP((A - sigma * M).tocsr())
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(rtol=1e-10)
    products = [0]

    def fwd(q):  # -sigma keep C^-1 M q
        return -sigma * keep * ksp.solve(np.asarray(M @ q, dtype=np.float64)).as_array().real

    def adj(q):  # -sigma M keep C^-T q
        return -sigma * (M @ (keep * ksp.solve_many(np.asarray(q, dtype=np.float64).reshape(n, 1), adjoint=True)[:, 0].real))

    def S(y):
        products[0] += 1
        q = np.zeros(n)
        q[u] = y
        for _ in range(steps):  # Phi q; sdirk2: one time step is s (a s + b) of the Euler-type step s
            q = fwd(SDIRK_A * fwd(q) + SDIRK_B * q) if two else fwd(q)
        q = M @ q
        for _ in range(steps):  # Phi^T (M Phi q), Phi^T = (-sigma M C^-T)^N; sdirk2: (a s^T + b) s^T
            if two:
                q = adj(q)
                q = SDIRK_A * adj(q) + SDIRK_B * q
            else:
                q = adj(q)
        return q[u]

    t1 = time.perf_counter()
    S(np.ones(u.size))  # orders, analyses, factorises
    t2 = time.perf_counter()
    v0 = np.random.default_rng(0).standard_normal(u.size)
    theta = spla.eigsh(spla.LinearOperator((u.size, u.size), matvec=S, dtype=np.float64), k=MODES, M=Muu, ncv=NCV, which="LA", tol=TOL, v0=v0,
                       return_eigenvectors=False)
    t3 = time.perf_counter()
    ksp.reset()
    return {"gains": np.sort(theta)[::-1], "seconds": time.perf_counter() - t0, "seconds_setup": t1 - t0, "seconds_first_product": t2 - t1,
            "seconds_iteration": t3 - t2, "products": products[0] - 1, "seconds_per_product": (t3 - t2) / max(products[0] - 1, 1),
            "read_backs_per_product": (4 if two else 2) * steps}


def windows_ab(cases, reps: int) -> dict:
    out = {"config": {"dt": DT, "horizon": HORIZON, "num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": reps, "scheme": SCHEME,
                      "response_strip": RESPONSE_STRIP}, "cases": []}
    for case in cases:
        if case.startswith("C"):
            continue  # (the strip is the cylinder's)
        es = problem(case)
        settings = {"plain": False, "ones": "ones", "windowed": True}
        warm = {name: library(es, w) for name, w in settings.items()}
        runs = {name: [] for name in settings}
        for _ in range(reps):
            for name, w in settings.items():
                runs[name].append(library(es, w))
        entry = {"case": case, "n": int(es.A.shape[0]),
                 **{name: {"gains": warm[name]["gains"].tolist(), "seconds": spread([r["seconds"] for r in runs[name]]),
                           "seconds_per_step": spread([r["seconds_per_step"] for r in runs[name]]), "applies": warm[name]["applies"],
                           "restarts": warm[name]["restarts"], "refinements": warm[name]["refinements"]} for name in settings}}
        entry["per_step_ratio_median"] = entry["windowed"]["seconds_per_step"]["median"] / entry["plain"]["seconds_per_step"]["median"]
        entry["per_step_ratio_ones_median"] = entry["ones"]["seconds_per_step"]["median"] / entry["plain"]["seconds_per_step"]["median"]
        entry["ones_same_gains"] = bool(np.array_equal(warm["ones"]["gains"], warm["plain"]["gains"]))
        out["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    return out


def plain(run: dict) -> dict:
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in run.items()}


def spread(values) -> dict:
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["S30k", "C160k"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("library", "host"), default=None, help="one setting alone, once per case (for a kernel trace)")
    ap.add_argument("--scheme", choices=("euler", "sdirk2"), default="euler")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "growth_ab.json")
    ap.add_argument("--windows", action="store_true", help="the windowed solve against the plain one -> key growth of profiles/windows_ab.json")
    args = ap.parse_args(argv)
    global SCHEME
    SCHEME = args.scheme
    if args.windows:
        path = ROOT / "profiles" / "windows_ab.json"
        doc = json.loads(path.read_text()) if path.exists() else {}
        doc["growth"] = windows_ab(args.cases, args.reps)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(doc, indent=1) + "\n")
        return
    settings = {"library": library, "host": host}
    if args.only:
        for case in args.cases:
            print(json.dumps({"case": case, args.only: plain(settings[args.only](problem(case)))}), flush=True)
        return
    result = {"config": {"dt": DT, "horizon": HORIZON, "num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": args.reps, "scheme": SCHEME}, "cases": []}
    for case in args.cases:
        es = problem(case)
        warm = {name: fn(es) for name, fn in settings.items()}  # warm-up: code objects, buffers
        runs = {name: [] for name in settings}
        for _ in range(args.reps):
            for name, fn in settings.items():
                runs[name].append(fn(es))
        a, b = warm["library"]["gains"], warm["host"]["gains"]
        entry = {"case": case, "n": int(es.A.shape[0]),
                 "gain_difference": float(np.abs(a - b).max() / a[0]) if a.shape == b.shape else None,
                 "library": {"seconds": spread([r["seconds"] for r in runs["library"]]),
                             "seconds_per_step": spread([r["seconds_per_step"] for r in runs["library"]]), "last": plain(runs["library"][-1])},
                 "host": {"seconds": spread([r["seconds"] for r in runs["host"]]),
                          "seconds_per_product": spread([r["seconds_per_product"] for r in runs["host"]]), "last": plain(runs["host"][-1])}}
        entry["speedup_median"] = entry["host"]["seconds"]["median"] / entry["library"]["seconds"]["median"]
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    if SCHEME != "euler":  # beside the Euler rows of the same file
        kept = json.loads(args.out.read_text()) if args.out.exists() else {}
        kept[SCHEME] = result
        result = kept
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
