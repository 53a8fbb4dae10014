"""Stochastic forcing: the library's iteration on kept factor sets against what a user can drive from the host on kept factors.

    python tools/stochastic_ab.py [--cases S30k C160k] [--nodes 8 16] [--reps 3] [--out profiles/stochastic_ab.json]
    python tools/stochastic_ab.py --trace P [--reps 3] [--out profiles/stochastic_trace.json]

``library`` (a): ``Solver.stochastic.StochasticForcingSolver.solve`` -- set-up, ``nodes`` factorisations of ``A - i omega_k M`` on one
analysis, the real thick-restart Lanczos iteration on ``S = (1 / pi) sum_k w_k Re W(i omega_k)`` with all ``2 nodes`` inner solves of a step,
their checks and the orthogonalisation on the device, one read-back per step; then one apply per mode for the spectrum.
``library_batch`` (a'): the same with ``batch_forward=True`` (the forward solves of a step through the batched sweeps; same bits).
``library_batch_both`` (a''): ``batch_forward=True, batch_adjoint=True`` (the adjoint solves through the batched transposed sweeps and
their check products 16 per launch as well; same bits).  Its figures are ratios to ``library_batch`` OF THE SAME RUN: the per-step
time, and the adjoint sweeps and adjoint check products of all steps and applies from the handle's HIP events.
``host`` (b): ARPACK on a ``LinearOperator`` whose product calls ``nodes`` kept ``iKSP`` factorisations on the same device
(``solve_many(adjoint=True)``, a product with ``M`` in scipy, ``solve``, per node: two host round trips per node and product) and sums
the real parts on the host.  ``S`` is self-adjoint in the ``M``-inner product, not in the Euclidean one ARPACK's symmetric driver
assumes, and ``M`` is singular (no ``M^(1/2)``, no ``M^-1``), so (b) runs the general driver ``eigs`` on ``S`` and takes the real parts, as
``tools/resolvent_ab.py`` does.

num_modes 4, ncv 24, tolerance 1e-8, Gauss-Legendre on the band [0, 1.5].  Every timed sample builds its solver anew (construction,
preparation, factorisations, iteration, release inside the clock); the settings alternate in one process after one warm-up of each;
medians and spread over ``reps`` samples.  The variances of (a') are compared with those of (a) bit for bit, those of (b) in
relative size.  No test asserts these times.

``--trace P``: the total variance by ``P`` block probes.  ``library``: one ``lsa_stochastic_trace`` call (two independent columns per probe
through one direction's block sweeps on runs of up to 16 factor sets, one read-back per batch of probes).  ``host_loop``: ``P`` calls of
``basis.apply`` from Python (``2 nodes`` dependent solves and one synchronisation each) with ``z^T (S z)`` evaluated in numpy.  Both on
the SAME handle -- the same kept factor sets -- and the same probes (the generator's, seed 0); the factorisations are outside both
clocks.  S30k at 8 and 16 nodes and C160k at 8 nodes; after one warm-up of each the two alternate ``reps`` times; medians, the spread, the
ratio of the medians, the largest difference between the two sets of forms, and the library's phase split from its stats.
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

MODES, NCV, TOL, BAND = 4, 24, 1e-8, (0.0, 1.5)


def problem(case: str):
    from synthetic import fem

    return fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)


def library(es, nodes: int, batch: bool = False, batch_adjoint: bool = False) -> dict:
    from Solver.stochastic import StochasticConfig, StochasticForcingSolver

    t0 = time.perf_counter()
    sf = StochasticForcingSolver(es.A, es.M, StochasticConfig(num_modes=MODES, ncv=NCV, atol=TOL, nodes=nodes), batch_forward=batch,
                                 batch_adjoint=batch_adjoint)
    res = sf.solve(band=BAND)
    sf.release()
    st = res.stats
    return {"variances": res.variances, "seconds": time.perf_counter() - t0, "seconds_factor": st["seconds_factor"],
            "seconds_steps": st["seconds_expand"], "seconds_sweeps_device": st["seconds_solve"], "seconds_products_device": st["seconds_product"],
            "seconds_adjoint_sweeps_device": st["seconds_solve_adjoint"], "seconds_adjoint_products_device": st["seconds_product_adjoint"],
            "adjoint_batches": st["adjoint_batches"], "forward_batches": st["forward_batches"],
            "seconds_host_dense": st["seconds_dense"], "applies": st["applies"], "restarts": st["restarts"], "refinements": st["refinements"],
            "seconds_per_step": st["seconds_expand"] / max(st["applies"], 1), "bytes": st["stochastic_bytes"]}


def host(es, nodes: int) -> dict:
    from Solver.stochastic import gauss_legendre_band
    from Solver.utils import KSPType, PreconditionerType, iKSP

    t0 = time.perf_counter()
    A, M = sp.csr_matrix(es.A), sp.csr_matrix(es.M)
    om, w = gauss_legendre_band(*BAND, nodes)
    n = A.shape[0]
    ksps = []
    for omega in om:
        ksp = iKSP((A - 1j * omega * M).tocsr())
        ksp.set_type(KSPType.PREONLY)
        ksp.set_preconditioner(PreconditionerType.LU)
        ksp.set_tolerances(rtol=1e-10)
        ksps.append(ksp)
    products = [0]

    def S(v):
        products[0] += 1
        rhs = np.asarray(M @ v.real, dtype=np.complex128).reshape(n, 1)
        y = np.zeros(n)
        for ksp, wk in zip(ksps, w):
            z = ksp.solve_many(rhs, adjoint=True)[:, 0]
            y += (wk / np.pi) * ksp.solve(np.asarray(M @ z, dtype=np.complex128)).as_array().real
        return y

    t1 = time.perf_counter()
    S(np.ones(n))  # orders, analyses, factorises every node
    t2 = time.perf_counter()
    v0 = np.random.default_rng(0).standard_normal(n)
    theta = spla.eigs(spla.LinearOperator((n, n), matvec=S, dtype=np.float64), k=MODES, ncv=NCV, which="LM", tol=TOL, v0=v0, return_eigenvectors=False)
    t3 = time.perf_counter()
    for ksp in ksps:
        ksp.reset()
    return {"variances": np.sort(theta.real)[::-1], "seconds": time.perf_counter() - t0, "seconds_setup": t1 - t0, "seconds_first_product": t2 - t1,
            "seconds_iteration": t3 - t2, "products": products[0] - 1, "seconds_per_product": (t3 - t2) / max(products[0] - 1, 1)}


def trace_ab(case: str, nodes: int, probes: int, reps: int) -> dict:
    import lsa_hip
    from Solver.stochastic import StochasticConfig, StochasticForcingSolver, gauss_legendre_band, trace_summary

    es = problem(case)
    sf = StochasticForcingSolver(es.A, es.M, StochasticConfig(num_modes=MODES, ncv=NCV, atol=TOL, nodes=nodes))
    om, w = gauss_legendre_band(*BAND, nodes)
    prep, ctx, perm = sf._prepare(complex(0.0, max(float(om.max()), 1.0)))
    basis = lsa_hip.StochasticBasis(ctx, prep["dA"], prep["dM"], 1j * om, w, 1, ksp_rtol=sf._ksp_rtol)
    try:
        basis.set_row_permutation(perm)
        basis.set_batch_forward(True)  # (what the front end's applies run with)
        Z = basis.probes(probes, seed=0)
        Zown = np.ascontiguousarray(Z[perm].T)  # (apply takes the matrices' own numbering)

        def library():
            t0 = time.perf_counter()
            out = basis.trace(probes, probes=Z)
            return time.perf_counter() - t0, out["forms"], out["stats"]

        def host_loop():
            t0 = time.perf_counter()
            forms = np.array([v @ basis.apply(v)[0] for v in Zown])
            return time.perf_counter() - t0, forms, None

        library(), host_loop()  # warm-up: code objects, the sweeps' column buffers
        lib, loop = [], []
        for _ in range(reps):
            lib.append(library())
            loop.append(host_loop())
    finally:
        del basis
        sf.release()
    fa, fb, st = lib[-1][1], loop[-1][1], lib[-1][2]
    summary = trace_summary(fa)
    entry = {"case": case, "n": int(es.A.shape[0]), "nodes": nodes, "probes": probes, "library_seconds": spread([r[0] for r in lib]),
             "host_loop_seconds": spread([r[0] for r in loop]), "forms_max_relative_difference": float(np.abs(fa - fb).max() / np.abs(fb).max()),
             "total": summary["total"], "stderr": summary["stderr"], "library_stats": st,
             "library_phase_seconds": {"solve": st["seconds_solve"], "product": st["seconds_product"], "forms": st["seconds_forms"]}}
    entry["host_loop_over_library_median"] = entry["host_loop_seconds"]["median"] / entry["library_seconds"]["median"]
    return entry


def plain(run: dict) -> dict:
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in run.items()}


def spread(values) -> dict:
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["S30k", "C160k"])
    ap.add_argument("--nodes", nargs="+", type=int, default=[8, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="the library settings alone")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "stochastic_ab.json")
    ap.add_argument("--trace", type=int, default=None, metavar="P", help="the trace estimator against a host loop of P applies instead")
    args = ap.parse_args(argv)
    if args.trace is not None:
        out = args.out if args.out != ROOT / "profiles" / "stochastic_ab.json" else ROOT / "profiles" / "stochastic_trace.json"
        result = {"config": {"band": BAND, "probes": args.trace, "seed": 0, "reps": args.reps}, "cases": []}
        for case, N in (("S30k", 8), ("S30k", 16), ("C160k", 8)):
            result["cases"].append(trace_ab(case, N, args.trace, args.reps))
            print(json.dumps(result["cases"][-1]), flush=True)
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text(json.dumps(result, indent=1) + "\n")
        return
    settings = {"library": lambda es, N: library(es, N), "library_batch": lambda es, N: library(es, N, True),
                "library_batch_both": lambda es, N: library(es, N, True, True)}
    if not args.no_host:
        settings["host"] = host
    result = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "band": BAND, "reps": args.reps}, "cases": []}
    for case in args.cases:
        es = problem(case)
        for N in args.nodes:
            warm = {name: fn(es, N) for name, fn in settings.items()}  # warm-up: code objects, buffers
            runs = {name: [] for name in settings}
            for _ in range(args.reps):
                for name, fn in settings.items():
                    runs[name].append(fn(es, N))
            a = warm["library"]["variances"]
            entry = {"case": case, "n": int(es.A.shape[0]), "nodes": N, "variances": a.tolist(),
                     "batch_bit_identical": bool(np.array_equal(a, warm["library_batch"]["variances"])),
                     "batch_both_bit_identical": bool(np.array_equal(a, warm["library_batch_both"]["variances"]))}
            for name in settings:
                entry[name] = {"seconds": spread([r["seconds"] for r in runs[name]]), "last": plain(runs[name][-1])}
                if name != "host":
                    entry[name]["seconds_per_step"] = spread([r["seconds_per_step"] for r in runs[name]])
                    for key in ("seconds_adjoint_sweeps_device", "seconds_adjoint_products_device"):
                        entry[name][key] = spread([r[key] for r in runs[name]])
            entry["batch_per_step_ratio_median"] = entry["library_batch"]["seconds_per_step"]["median"] / entry["library"]["seconds_per_step"]["median"]
            both, base = entry["library_batch_both"], entry["library_batch"]  # (same steps on both sides: the bits are the same)
            entry["batch_both_ratios_to_library_batch_median"] = {
                "per_step": both["seconds_per_step"]["median"] / base["seconds_per_step"]["median"],
                "adjoint_sweeps": both["seconds_adjoint_sweeps_device"]["median"] / base["seconds_adjoint_sweeps_device"]["median"],
                "adjoint_products": both["seconds_adjoint_products_device"]["median"] / base["seconds_adjoint_products_device"]["median"]}
            if "host" in settings:
                b = warm["host"]["variances"]
                entry["variance_difference"] = float(np.abs(a - b).max() / a[0]) if a.shape == b.shape else None
                entry["speedup_median"] = entry["host"]["seconds"]["median"] / entry["library"]["seconds"]["median"]
            result["cases"].append(entry)
            print(json.dumps(entry), flush=True)
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
