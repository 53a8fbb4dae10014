"""Region eigensolver against Krylov-Schur at the region's centre: what the completeness statement costs.

    python tools/region_ab.py [--cases S30k] [--inside 15] [--subspace 48] [--nodes 16] [--reps 3] [--out profiles/region_ab.json]

Per case the region is a circle about the bench shift chosen on the CPU (``oracle.shift_invert``): its radius lies halfway between
the ``inside``-th and the next nearest eigenvalue, so that ``inside`` eigenvalues lie inside and ``subspace - inside`` directions are
spare (at least 12 asked for).  Alternating, after one warm-up of each, fresh solvers per sample and the host clock from construction
to release: (a) ``RegionEigenSolver`` with kept factor sets, (b) with one refactorised set, (c) ``EigenSolver`` (Krylov-Schur,
shift-invert at ``target = centre``, ``nev`` = the count), which finds the same pairs without the proof.  Medians and spreads of
``reps`` samples; for (a) and (b) also the split factor / block solves / products / Gram / host dense of ``lsa_contour_info`` and the
iterations.  ``--batch-nodes`` adds one more row, (d) kept factor sets with the nodes solved in lockstep
(``RegionConfig(batch_nodes=True)``): the same regions in the same process, so that ``seconds_solve`` and the wall time stand beside
those of (a), the switch off; ``--skip-krylov`` leaves (b) and (c) out for that comparison alone.

``--two-sided`` measures the left phase instead (``RegionConfig(two_sided=True)``, kept factor sets): (e) the two-sided solve with
``batch_nodes`` off and (f) on -- the left phase's ``seconds_solve`` of both stand side by side --, and (g) what the left vectors cost
without it: a right solve plus a fresh ``RegionEigenSolver(A^H, M^T)`` on the conjugate region, which factorises again.  The case is
merged into ``profiles/multi_batch_adjoint.json`` under ``"region_two_sided"`` unless ``--out`` says otherwise.  Needs an AMD GPU.
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

SPLIT = ("seconds_factor", "seconds_solve", "seconds_product", "seconds_gram", "seconds_dense")


def choose_circle(es, centre: complex, inside: int, subspace: int):
    from oracle import shift_invert

    lam, _, _ = shift_invert.solve(es.A, es.M, centre, k=inside + 6, tol=1e-10, ncv=max(4 * inside, 80))
    d = np.sort(np.abs(np.asarray(lam) - centre))
    if subspace - inside < 12:
        raise SystemExit(f"subspace {subspace} leaves fewer than 12 spare directions beside {inside} eigenvalues")
    return 0.5 * float(d[inside - 1] + d[inside]), float(d[inside - 1]), float(d[inside])


def region_sample(es, centre, radius, cfg_args, keep: bool, batch_nodes: bool = False, two_sided: bool = False, adjoint_pencil: bool = False) -> dict:
    from Solver.region import Ellipse, RegionConfig, RegionEigenSolver

    t0 = time.perf_counter()
    A, M = (es.A.conj().T.tocsr(), es.M.T.tocsr()) if adjoint_pencil else (es.A, es.M)
    rs = RegionEigenSolver(A, M, RegionConfig(keep_factors=keep, batch_nodes=batch_nodes, two_sided=two_sided, **cfg_args))
    res = rs.solve(Ellipse(centre.conjugate() if adjoint_pencil else centre, radius, radius))
    rs.release()
    dt = time.perf_counter() - t0
    left = {f"left_{k}": v for k, v in res.stats.get("left", {}).items()}
    if two_sided:
        left.update(left_complete=bool(res.left_complete), kappa_max=float(np.max(res.condition_numbers, initial=0.0)) if res.left_complete else None)
    return {**left, "seconds": dt, "count": res.count, "complete": res.complete, "iterations": res.iterations, "max_residual": float(np.max(res.residuals, initial=0.0)),
            "refined_solves": res.stats["refined_solves"], "block_solves": res.stats["block_solves"], "eigenvalues": res.eigenvalues,
            "batched_groups": res.stats["batched_groups"], "batched_columns": res.stats["batched_columns"],
            **{k: res.stats[k] for k in SPLIT}}


def krylov_sample(es, centre, nev: int, atol: float) -> dict:
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    t0 = time.perf_counter()
    s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=nev, atol=atol, ncv=max(2 * nev, nev + 15)), check_hermitian=False)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(centre)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    pairs = s.solve()
    st = dict(s.solver.stats)
    s.solver.release()
    dt = time.perf_counter() - t0
    return {"seconds": dt, "pairs": len(pairs), "applies": st["op_applies"], "restarts": st["krylov_restarts"], "seconds_factor": st["seconds_factor"],
            "eigenvalues": np.array([p[0] for p in pairs])}


def summarise(runs: list[dict], keys) -> dict:
    out = {k: v for k, v in runs[0].items() if k not in keys and k not in ("seconds", "eigenvalues")}
    for k in ("seconds",) + tuple(keys):
        v = [r[k] for r in runs]
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return out


LEFT_SPLIT = ("left_seconds_solve", "left_seconds_product", "left_seconds_gram", "left_seconds_dense")


def two_sided_case(name, es, centre, radius, cfg_args, reps: int) -> dict:
    """Medians of: the two-sided solve with batch_nodes off / on, and a right solve followed by a fresh solver on (A^H, M^T)."""
    def separate():
        a = region_sample(es, centre, radius, cfg_args, True)
        b = region_sample(es, centre, radius, cfg_args, True, adjoint_pencil=True)
        return {"seconds": a["seconds"] + b["seconds"], "count": a["count"], "adjoint_count": b["count"],
                **{k: a[k] + b[k] for k in SPLIT}, "eigenvalues": a["eigenvalues"]}

    samplers = {"two_sided": lambda: region_sample(es, centre, radius, cfg_args, True, False, True),
                "two_sided_batch_nodes": lambda: region_sample(es, centre, radius, cfg_args, True, True, True),
                "right_plus_adjoint_solver": separate}
    runs = {k: [] for k in samplers}
    for fn in samplers.values():
        fn()
    for _ in range(reps):
        for k, fn in samplers.items():
            runs[k].append(fn())
    case = {"case": name, "n": int(es.n), "centre": [centre.real, centre.imag], "radius": radius,
            "two_sided": summarise(runs["two_sided"], SPLIT + LEFT_SPLIT), "two_sided_batch_nodes": summarise(runs["two_sided_batch_nodes"], SPLIT + LEFT_SPLIT),
            "right_plus_adjoint_solver": summarise(runs["right_plus_adjoint_solver"], SPLIT)}
    case["left_seconds_solve_off_over_on"] = case["two_sided"]["left_seconds_solve"]["median"] / case["two_sided_batch_nodes"]["left_seconds_solve"]["median"]
    case["separate_over_two_sided"] = case["right_plus_adjoint_solver"]["seconds"]["median"] / case["two_sided"]["seconds"]["median"]
    print(json.dumps(case), flush=True)
    return case


def main(argv=None) -> None:
    from synthetic import fem

    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["S30k"])
    ap.add_argument("--inside", type=int, default=15)
    ap.add_argument("--subspace", type=int, default=48)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--atol", type=float, default=1e-10)
    ap.add_argument("--max-it", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-nodes", action="store_true", help="one more row: kept factor sets, the nodes solved in lockstep")
    ap.add_argument("--skip-krylov", action="store_true", help="only the kept rows (with --batch-nodes: the switch off and on)")
    ap.add_argument("--two-sided", action="store_true", help="the left phase with batch_nodes off and on, and a right solve plus a fresh solver on the adjoint pencil")
    ap.add_argument("--out", type=Path, default=None, help="default: profiles/region_ab.json; with --two-sided profiles/multi_batch_adjoint.json (merged)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = ROOT / "profiles" / ("multi_batch_adjoint.json" if args.two_sided else "region_ab.json")
    cfg_args = {"nodes": args.nodes, "subspace": args.subspace, "atol": args.atol, "max_it": args.max_it}
    result = {"config": {**cfg_args, "inside": args.inside, "reps": args.reps}, "cases": []}
    for name in args.cases:
        cube = name.startswith("C")
        es = fem.cube_case(name) if cube else fem.cylinder_case(name)
        centre = complex(fem.SIGMA_CUBE if cube else fem.SIGMA_RE50)
        radius, d_in, d_out = choose_circle(es, centre, args.inside, args.subspace)
        if args.two_sided:
            result["cases"].append(two_sided_case(name, es, centre, radius, cfg_args, args.reps))
            continue
        samplers = {"kept": lambda: region_sample(es, centre, radius, cfg_args, True),
                    "refactorised": lambda: region_sample(es, centre, radius, cfg_args, False),
                    "krylov_schur": lambda: krylov_sample(es, centre, args.inside, args.atol)}
        if args.batch_nodes:
            samplers["kept_batch_nodes"] = lambda: region_sample(es, centre, radius, cfg_args, True, True)
        if args.skip_krylov:
            samplers = {k: fn for k, fn in samplers.items() if k.startswith("kept")}
        runs = {k: [] for k in samplers}
        for fn in samplers.values():
            fn()  # warm-up: code objects, host caches
        for _ in range(args.reps):
            for k, fn in samplers.items():
                runs[k].append(fn())
        lam_r = runs["kept"][0]["eigenvalues"]
        case = {"case": name, "n": int(es.n), "centre": [centre.real, centre.imag], "radius": radius, "nearest_inside": d_in, "nearest_outside": d_out,
                "kept": summarise(runs["kept"], SPLIT)}
        if "kept_batch_nodes" in runs:
            case["kept_batch_nodes"] = summarise(runs["kept_batch_nodes"], SPLIT)
            case["batch_nodes_same_bytes"] = bool(runs["kept_batch_nodes"][0]["eigenvalues"].tobytes() == lam_r.tobytes())
            case["seconds_solve_off_over_on"] = case["kept"]["seconds_solve"]["median"] / case["kept_batch_nodes"]["seconds_solve"]["median"]
        if not args.skip_krylov:
            lam_k = runs["krylov_schur"][0]["eigenvalues"]
            inside_k = lam_k[np.abs(lam_k - centre) < radius]
            diff = max((float(np.min(np.abs(lam_r - z))) for z in inside_k), default=float("nan")) if lam_r.size else float("nan")
            case.update(refactorised=summarise(runs["refactorised"], SPLIT), krylov_schur=summarise(runs["krylov_schur"], ("seconds_factor",)),
                        krylov_inside=int(inside_k.size), eigenvalue_difference=diff)
            case["proof_cost_ratio"] = case["kept"]["seconds"]["median"] / case["krylov_schur"]["seconds"]["median"]
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    if args.two_sided:  # merged into the document of tools/multi_rhs_throughput.py --sets J --trans H
        doc = json.loads(args.out.read_text()) if args.out.exists() else {}
        doc["region_two_sided"] = result
        result = doc
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
