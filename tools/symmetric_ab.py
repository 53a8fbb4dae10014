"""Symmetric-definite eigenproblems: the real thick-restart Lanczos path (``symmetric=True``) against the general complex path.

    python tools/symmetric_ab.py [--sizes 128 256 512] [--reps 3] [--out profiles/symmetric_ab.json]

Interior membrane pencils (``synthetic.fem.assemble_membrane`` on the square a = b = 2 with the boundary dofs removed and both
matrices symmetrised) at nx x nx cells: 65 k, 261 k and 1.05 M unknowns.  ``GHEP``, shift-invert at sigma = 0 with the exact
factorisation, nev = 24, ncv = 48, tol 1e-10.  ``symmetric`` off and on alternate in one process after one warm-up solve of each;
``reps`` timed solves per setting.  Per setting: medians and the spread (min, max) of the seconds per solve (factorisation +
iteration + vectors; the upload is prepared before the clock starts), operator applies, restarts, the library's time split
(``seconds_factor`` / ``seconds_expand`` / ``seconds_dense`` / ``seconds_restart``), ``basis_bytes`` and the device-memory
high-water mark (the device's used bytes by ``hipMemGetInfo``, sampled after each solve).
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

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

SPLIT = ("seconds_factor", "seconds_expand", "seconds_dense", "seconds_restart")


def interior_membrane(nx: int):
    from synthetic import fem

    A, M, bnd = fem.assemble_membrane(nx, nx, 2.0, 2.0)
    keep = np.setdiff1d(np.arange(A.shape[0]), bnd)
    out = []
    for X in (A, M):
        Xi = sp.csr_matrix(X)[keep][:, keep]
        Xi = sp.csr_matrix((Xi + Xi.T) * 0.5)
        Xi.sort_indices()
        out.append(Xi)
    return out


def build(K, M, symmetric: bool):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType

    s = EigenSolver(K, M, EigensolverConfig(num_eig=24, problem_type=iEpsProblemType.GHEP, atol=1e-10, ncv=48, max_it=500), check_hermitian=False,
                    symmetric=symmetric)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(0.0)
    s.solver.set_st_pc_type(PreconditionerType.CHOLESKY)
    return s


def device_used_bytes() -> int:
    """Used bytes of device 0 by ``hipMemGetInfo`` of the HIP runtime the library has loaded (-1 if it cannot be asked)."""
    import ctypes

    try:
        hip = ctypes.CDLL("libamdhip64.so")
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
            return -1
        return int(total.value - free.value)
    except OSError:
        return -1


def one_solve(s) -> dict:
    s.solver.prepare()
    t0 = time.perf_counter()
    pairs = s.solve()
    dt = time.perf_counter() - t0
    st = s.solver.stats
    return {"seconds": dt, "pairs": len(pairs), "method": st["method"], "applies": st["op_applies"], "restarts": st["krylov_restarts"],
            "basis_bytes": st["basis_bytes"], "device_used_bytes": device_used_bytes(), "max_residual": float(np.max(s.solver.residuals())),
            "fallback": st.get("symmetric_fallback"), **{k: st.get(k, 0.0) for k in SPLIT}}


def summarise(runs: list[dict]) -> dict:
    out = {"method": runs[0]["method"], "pairs": runs[0]["pairs"], "applies": runs[0]["applies"], "restarts": runs[0]["restarts"],
           "basis_bytes": runs[0]["basis_bytes"], "device_used_bytes_max": max(r["device_used_bytes"] for r in runs),
           "max_residual": max(r["max_residual"] for r in runs), "fallback": runs[0]["fallback"]}
    for k in ("seconds",) + SPLIT:
        v = [r[k] for r in runs]
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "symmetric_ab.json")
    args = ap.parse_args(argv)
    result = {"config": {"nev": 24, "ncv": 48, "tol": 1e-10, "sigma": 0.0, "reps": args.reps}, "cases": []}
    for nx in args.sizes:
        K, M = interior_membrane(nx)
        solvers = {flag: build(K, M, flag) for flag in (False, True)}
        runs = {False: [], True: []}
        for flag in (False, True):
            one_solve(solvers[flag])  # warm-up: analysis, buffers, code objects
        for _ in range(args.reps):
            for flag in (False, True):
                runs[flag].append(one_solve(solvers[flag]))
        lam = {flag: np.sort(np.real(solvers[flag].solver._eigenvalues[:24])) for flag in (False, True)}
        case = {"nx": nx, "n": int(K.shape[0]), "nnz": int(K.nnz), "general": summarise(runs[False]), "symmetric": summarise(runs[True]),
                "eigenvalue_difference": float(np.max(np.abs(lam[True] - lam[False]) / np.abs(lam[True])))}
        case["speedup_median"] = case["general"]["seconds"]["median"] / case["symmetric"]["seconds"]["median"]
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        for s in solvers.values():
            s.solver.release()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
