"""Optimal gains: the library's resolvent iteration against what a user can drive from the host on kept factors.

    python tools/resolvent_ab.py [--cases S30k C160k] [--reps 3] [--forcings] [--windows] [--out profiles/resolvent_ab.json]

``library`` (a): ``Solver.resolvent.ResolventSolver.solve`` -- set-up, one factorisation of ``A - i omega M``, the thick-restart Lanczos
iteration on ``W = C^-1 M C^-H M`` with both inner solves, their checks and the orthogonalisation on the device, one read-back per step.
``host`` (b): ARPACK on a ``LinearOperator`` whose product is ``iKSP.solve_many(adjoint=True)`` then ``iKSP.solve`` on ONE kept
factorisation of the same matrix, the two products with ``M`` in scipy: two host round trips and two host-side verifications per
product.  ``W`` is self-adjoint in the ``M``-inner product, not in the Euclidean one ARPACK's symmetric driver assumes, and ``M`` is
singular (no ``M^(1/2)``, no ``M^-1``), so (b) runs the general driver ``eigs`` on ``W`` and takes the real parts.

num_modes 6, ncv 32, tolerance 1e-8; omega = the imaginary part of the case's bench target (S30k: 0.738, C160k: 0, real factors).
Every timed sample builds its solver anew (construction, preparation, factorisation, iteration, release inside the clock); the two
settings alternate in one process after one warm-up of each; medians and spread over ``reps`` samples.  The gains of (b) are
compared with those of (a).  Launches and read-backs per step are counted from the step's code (``csrc/resolvent.hip``, ``csrc/lanczos.hip``), not timed;
the per-kernel times of the three step kernels come from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--only library``.
No test asserts these times.

``--forcings`` measures the forcings phase instead and records it under the key ``forcings_phase`` of the same file (the other keys
stay): ``ResolventSolver.solve`` without forcings, with them one adjoint solve at a time, and with ``block_forcings=True`` (one block
solve), alternately after a warm-up of each.  The figure is ``stats["seconds_restart"]``, the loop's phase that holds the thick restarts, the
Ritz vectors and, where asked for, the forcings: a setting's figure minus that of the run without forcings is its forcings phase.  The
forcings of the two settings are compared bit for bit.

``--windows`` compares the library's solve with a forcing window (x in [-3, 3], |y| <= 3) and a response window (x in [2, 30]) against
its plain solve and against the plain problem solved through windows of ones (the same iteration, step for step, with two
windowed copies of ``M`` in flight: the like-for-like figure), alternately after a warm-up of each (cylinder cases), and times the call that builds one windowed matrix
(``CsrMatrix.windowed``: the upload of the window, ``window_values_kernel`` and the synchronisation) on every case given; the result goes
under the key ``resolvent`` of ``profiles/windows_ab.json``.  The weighted step has the launches of the plain one, so the figure to
compare is ``seconds_per_step``; the iteration counts differ, since the windowed problem is another problem.

``--lockstep J`` times a sweep of J distinct frequencies three ways in the same process, fresh solvers for each, alternately after a
warm-up of each: the sequential ``sweep`` (the default path: the baseline), ``sweep(lockstep=True)`` and the host-driven ARPACK loop.
Per frequency it reports the factor / step / host-dense / restart-and-forcings split from the stats, plus rounds and launches per
round, and whether the lockstep sweep returned the sequential one's bytes; the rows go to ``profiles/resolvent_lockstep.json``.
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

MODES, NCV, TOL = 6, 32, 1e-8


def problem(case: str):
    from synthetic import fem

    if case.startswith("C"):
        return fem.cube_case(case), float(complex(fem.SIGMA_CUBE).imag)
    return fem.cylinder_case(case), float(complex(fem.SIGMA_RE50).imag)


FORCING_BOX, RESPONSE_STRIP = (-3.0, 3.0, -3.0, 3.0), (2.0, 30.0)


def cylinder_windows(es):
    """The 0/1 forcing and response windows of a cylinder case."""
    x, y = es.dof_xy()
    fx0, fx1, fy0, fy1 = FORCING_BOX
    return (((x >= fx0) & (x <= fx1) & (y >= fy0) & (y <= fy1)).astype(float), ((x >= RESPONSE_STRIP[0]) & (x <= RESPONSE_STRIP[1])).astype(float))


def library(es, omega: float, windows=False) -> dict:
    from Solver.resolvent import ResolventConfig, ResolventSolver

    t0 = time.perf_counter()
    kw = {}
    if windows == "ones":  # the plain problem through two windowed copies of M: the same iteration, two more matrices in flight
        kw = dict(forcing_window=np.ones(es.n), response_window=np.ones(es.n))
    elif windows:
        kw = dict(zip(("forcing_window", "response_window"), cylinder_windows(es)))
    rs = ResolventSolver(es.A, es.M, ResolventConfig(num_modes=MODES, ncv=NCV, atol=TOL), **kw)
    rs.solver.set_target(complex(0.0, omega))
    rs.solver.prepare()
    t1 = time.perf_counter()
    res = rs.solve(omega, forcings=False)
    t2 = time.perf_counter()
    rs.release()
    st = res.stats
    steps = max(st["applies"], 1)
    return {"gains": res.gains, "seconds": time.perf_counter() - t0, "seconds_setup": t1 - t0, "seconds_solve_call": t2 - t1,
            "seconds_factor": st["seconds_factor"], "seconds_steps": st["seconds_expand"], "seconds_host_dense": st["seconds_dense"],
            "seconds_restart": st["seconds_restart"], "applies": st["applies"], "restarts": st["restarts"],
            "refinements": st["refinements"], "seconds_per_step": st["seconds_expand"] / steps, "read_backs_per_step": 1}


def host(es, omega: float) -> dict:
    from Solver.utils import KSPType, PreconditionerType, iKSP

    t0 = time.perf_counter()
    A, M = sp.csr_matrix(es.A), sp.csr_matrix(es.M)
    C = (A - 1j * omega * M).tocsr() if omega != 0.0 else A
    ksp = iKSP(C)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(rtol=1e-10)
    n = A.shape[0]
    products = [0]

    def W(v):
        products[0] += 1
        z = ksp.solve_many(np.asarray(M @ v, dtype=np.complex128).reshape(n, 1), adjoint=True)[:, 0]
        return ksp.solve(np.asarray(M @ z, dtype=np.complex128)).as_array()

    t1 = time.perf_counter()
    W(np.ones(n, dtype=np.complex128))  # orders, analyses, factorises
    t2 = time.perf_counter()
    rng = np.random.default_rng(0)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    theta = spla.eigs(spla.LinearOperator((n, n), matvec=W, dtype=np.complex128), k=MODES, ncv=NCV, which="LM", tol=TOL, v0=v0,
                      return_eigenvectors=False)
    t3 = time.perf_counter()
    ksp.reset()
    gains = np.sqrt(np.sort(theta.real)[::-1])
    return {"gains": gains, "seconds": time.perf_counter() - t0, "seconds_setup": t1 - t0, "seconds_first_product": t2 - t1,
            "seconds_iteration": t3 - t2, "products": products[0] - 1, "seconds_per_product": (t3 - t2) / max(products[0] - 1, 1),
            "read_backs_per_product": 2}


def forcings_run(es, omega: float, forcings: bool, block: bool) -> dict:
    from Solver.resolvent import ResolventConfig, ResolventSolver

    rs = ResolventSolver(es.A, es.M, ResolventConfig(num_modes=MODES, ncv=NCV, atol=TOL), block_forcings=block)
    res = rs.solve(omega, forcings=forcings)
    rs.release()
    st = res.stats
    return {"forcings": res.forcings, "gains": res.gains, "seconds_restart": st["seconds_restart"], "seconds_steps": st["seconds_expand"],
            "adjoint_solves": st["adjoint_solves"], "refined_adjoint": st["refined_adjoint"]}


def forcings_phase(cases, reps: int) -> dict:
    settings = {"none": (False, False), "one_by_one": (True, False), "block": (True, True)}
    out = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": reps}, "cases": []}
    for case in cases:
        es, omega = problem(case)
        warm = {name: forcings_run(es, omega, *flags) for name, flags in settings.items()}
        runs = {name: [] for name in settings}
        for _ in range(reps):
            for name, flags in settings.items():
                runs[name].append(forcings_run(es, omega, *flags)["seconds_restart"])
        med = {name: statistics.median(v) for name, v in runs.items()}
        entry = {"case": case, "n": int(es.A.shape[0]), "omega": omega, "columns": int(len(warm["block"]["gains"])),
                 "bit_identical": bool(np.array_equal(warm["one_by_one"]["forcings"], warm["block"]["forcings"])),
                 "adjoint_solves": [warm["one_by_one"]["adjoint_solves"], warm["block"]["adjoint_solves"]],
                 "refined_adjoint": [warm["one_by_one"]["refined_adjoint"], warm["block"]["refined_adjoint"]],
                 "seconds_restart": {name: spread(v) for name, v in runs.items()},
                 "forcings_seconds_one_by_one": med["one_by_one"] - med["none"], "forcings_seconds_block": med["block"] - med["none"]}
        out["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    return out


def window_call_seconds(es, reps: int) -> dict:
    """Wall-clock seconds of ``CsrMatrix.windowed`` on the case's M (a smooth window: the time does not depend on the values)."""
    import lsa_hip

    ctx = lsa_hip.Context(0)
    M = sp.csr_matrix(es.M)
    dM = lsa_hip.CsrMatrix.from_scipy(ctx, M)
    d = 0.5 * (1.0 + np.tanh(np.linspace(-3.0, 3.0, M.shape[0])))
    dM.windowed(d)  # warm-up: the code object
    times = []
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        W = dM.windowed(d)
        times.append(time.perf_counter() - t0)
        del W
    del dM
    ctx.close()
    return {"n": int(M.shape[0]), "nnz": int(M.nnz), "seconds": spread(times)}


def windows_ab(cases, reps: int) -> dict:
    out = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": reps, "forcing_box": FORCING_BOX, "response_strip": RESPONSE_STRIP},
           "cases": [], "window_call": []}
    for case in cases:
        es, omega = problem(case)
        out["window_call"].append({"case": case, **window_call_seconds(es, reps)})
        print(json.dumps(out["window_call"][-1]), flush=True)
        if case.startswith("C"):
            continue  # (the boxes are the cylinder's)
        settings = {"plain": False, "ones": "ones", "windowed": True}
        warm = {name: library(es, omega, w) for name, w in settings.items()}
        runs = {name: [] for name in settings}
        for _ in range(reps):
            for name, w in settings.items():
                runs[name].append(library(es, omega, w))
        entry = {"case": case, "n": int(es.A.shape[0]), "omega": omega,
                 **{name: {"gains": warm[name]["gains"].tolist(), "seconds": spread([r["seconds"] for r in runs[name]]),
                           "seconds_per_step": spread([r["seconds_per_step"] for r in runs[name]]),
                           "seconds_setup": spread([r["seconds_setup"] for r in runs[name]]), "applies": warm[name]["applies"],
                           "restarts": warm[name]["restarts"], "refinements": warm[name]["refinements"]} for name in settings}}
        entry["per_step_ratio_median"] = entry["windowed"]["seconds_per_step"]["median"] / entry["plain"]["seconds_per_step"]["median"]
        entry["per_step_ratio_ones_median"] = entry["ones"]["seconds_per_step"]["median"] / entry["plain"]["seconds_per_step"]["median"]
        entry["ones_same_gains"] = bool(np.array_equal(warm["ones"]["gains"], warm["plain"]["gains"]))
        out["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    return out


def sweep_frequencies(omega: float, J: int) -> list:
    """J distinct non-zero frequencies around the case's own (a case whose frequency is 0 sweeps 0.2 ... upwards)."""
    base = omega if omega != 0.0 else 0.2
    return [base * (0.6 + 0.8 * k / max(J - 1, 1)) for k in range(J)]


def sweep_run(es, omegas, lockstep: bool, max_batch: int = 16) -> dict:
    """One sweep on a fresh solver, construction to release: the per-frequency split from the stats."""
    from Solver.resolvent import ResolventConfig, ResolventSolver

    t0 = time.perf_counter()
    rs = ResolventSolver(es.A, es.M, ResolventConfig(num_modes=MODES, ncv=NCV, atol=TOL))
    res = rs.sweep(omegas, forcings=True, lockstep=lockstep, max_batch=max_batch)
    info = list(rs.last_lockstep_info)
    rs.release()
    J = len(omegas)
    tot = lambda key: sum(r.stats[key] for r in res)  # noqa: E731
    return {"seconds": time.perf_counter() - t0, "gains": [r.gains.tolist() for r in res], "responses": [r.responses for r in res],
            "forcings": [r.forcings for r in res],
            "per_frequency": {"factor": tot("seconds_factor") / J, "steps": tot("seconds_expand") / J, "host_dense": tot("seconds_dense") / J,
                              "restart_vectors_forcings": tot("seconds_restart") / J},
            "applies": [r.stats["applies"] for r in res], "lockstep_steps": [r.stats.get("lockstep_steps", 0) for r in res],
            "solo_steps": [r.stats.get("solo_steps", r.stats["applies"]) for r in res],
            "rounds": sum(i["rounds"] for i in info), "launches_per_round": (sum(i["launches"] for i in info) / max(sum(i["rounds"] for i in info), 1))}


def host_sweep(es, omegas) -> dict:
    """The host loop at every frequency; ``{"refused": text}`` where it cannot run one (``iKSP``'s factorisation has no re-analysis
    with constraints: a zero pivot inside a front ends it, where the operator build of the library analyses again)."""
    import lsa_hip

    t0 = time.perf_counter()
    try:
        runs = [host(es, w) for w in omegas]
    except lsa_hip.LsaError as exc:
        return {"refused": str(exc)}
    return {"seconds": time.perf_counter() - t0, "gains": [r["gains"].tolist() for r in runs],
            "per_frequency": {"setup_and_factor": sum(r["seconds_setup"] + r["seconds_first_product"] for r in runs) / len(runs),
                              "iteration": sum(r["seconds_iteration"] for r in runs) / len(runs)}}


def lockstep_ab(cases, reps: int, J: int) -> dict:
    """A sweep of J distinct frequencies three ways in one process -- the sequential ``sweep`` (the baseline: the default path), the
    lockstep ``sweep`` and the host-driven ARPACK loop --, fresh solvers for each, alternately after one warm-up of each."""
    out = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": reps, "frequencies": J}, "cases": []}
    for case in cases:
        es, omega = problem(case)
        omegas = sweep_frequencies(omega, J)
        settings = {"sequential": lambda: sweep_run(es, omegas, False), "lockstep": lambda: sweep_run(es, omegas, True, min(J, 16)),
                    "host": lambda: host_sweep(es, omegas)}
        # (where the device does not hold J factor sets the front end cuts the group: `rounds` and `lockstep_steps` show what ran together)
        warm = {name: fn() for name, fn in settings.items()}
        same = all(np.array_equal(a, b) for key in ("responses", "forcings") for a, b in zip(warm["sequential"][key], warm["lockstep"][key]))
        same = same and warm["sequential"]["gains"] == warm["lockstep"]["gains"]
        if "refused" in warm["host"]:  # (stated, and left out of the alternation)
            del settings["host"]
        runs = {name: [] for name in settings}
        for _ in range(reps):
            for name, fn in settings.items():
                runs[name].append(fn())
        strip = lambda r: {k: v for k, v in r.items() if k not in ("responses", "forcings", "gains")}  # noqa: E731
        entry = {"case": case, "n": int(es.A.shape[0]), "omegas": omegas, "lockstep_bytes_equal_sequential": bool(same),
                 **{name: {"seconds": spread([r["seconds"] for r in runs[name]]),
                           "per_frequency": {k: spread([r["per_frequency"][k] for r in runs[name]]) for k in runs[name][0]["per_frequency"]},
                           "last": strip(runs[name][-1])} for name in settings}}
        if "refused" in warm["host"]:
            entry["host"] = warm["host"]
        entry["sweep_speedup_median"] = entry["sequential"]["seconds"]["median"] / entry["lockstep"]["seconds"]["median"]
        entry["step_seconds_ratio_median"] = (entry["lockstep"]["per_frequency"]["steps"]["median"] /
                                              entry["sequential"]["per_frequency"]["steps"]["median"])
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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "resolvent_ab.json")
    ap.add_argument("--forcings", action="store_true", help="the forcings phase with block_forcings off and on -> key forcings_phase of --out")
    ap.add_argument("--windows", action="store_true", help="the windowed solve against the plain one -> key resolvent of profiles/windows_ab.json")
    ap.add_argument("--lockstep", type=int, default=0, metavar="J",
                    help="a sweep of J frequencies: sequential, lockstep and host loop -> key lockstep_J of profiles/resolvent_lockstep.json")
    args = ap.parse_args(argv)
    if args.lockstep:
        path = ROOT / "profiles" / "resolvent_lockstep.json"
        doc = json.loads(path.read_text()) if path.exists() else {}
        for entry in lockstep_ab(args.cases, args.reps, args.lockstep)["cases"]:
            doc[f"{entry['case']}_lockstep_{args.lockstep}"] = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": args.reps}, **entry}
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(doc, indent=1) + "\n")
        return
    if args.windows:
        path = ROOT / "profiles" / "windows_ab.json"
        doc = json.loads(path.read_text()) if path.exists() else {}
        doc["resolvent"] = windows_ab(args.cases, args.reps)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(doc, indent=1) + "\n")
        return
    if args.forcings:
        doc = json.loads(args.out.read_text()) if args.out.exists() else {}
        doc["forcings_phase"] = forcings_phase(args.cases, args.reps)
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(doc, indent=1) + "\n")
        return
    settings = {"library": library, "host": host}
    if args.only:
        for case in args.cases:
            es, omega = problem(case)
            print(json.dumps({"case": case, args.only: plain(settings[args.only](es, omega))}), flush=True)
        return
    result = {"config": {"num_modes": MODES, "ncv": NCV, "tol": TOL, "reps": args.reps}, "cases": []}
    for case in args.cases:
        es, omega = problem(case)
        warm = {name: fn(es, omega) for name, fn in settings.items()}  # warm-up: code objects, buffers
        runs = {name: [] for name in settings}
        for _ in range(args.reps):
            for name, fn in settings.items():
                runs[name].append(fn(es, omega))
        a, b = warm["library"]["gains"], warm["host"]["gains"]
        entry = {"case": case, "n": int(es.A.shape[0]), "omega": omega,
                 "gain_difference": float(np.abs(a - b).max() / a[0]) if a.shape == b.shape else None,
                 "library": {"seconds": spread([r["seconds"] for r in runs["library"]]),
                             "seconds_per_step": spread([r["seconds_per_step"] for r in runs["library"]]), "last": plain(runs["library"][-1])},
                 "host": {"seconds": spread([r["seconds"] for r in runs["host"]]),
                          "seconds_per_product": spread([r["seconds_per_product"] for r in runs["host"]]), "last": plain(runs["host"][-1])}}
        entry["speedup_median"] = entry["host"]["seconds"]["median"] / entry["library"]["seconds"]["median"]
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
