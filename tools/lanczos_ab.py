"""SHA-256 digests and counters of the three self-adjoint outer iterations (symmetric eigensolver, resolvent, transient growth),
as one JSON object (development aid): run it on two builds (``LSA_HIP_LIB`` picks the library) and compare the files -- a
refactoring of the Lanczos basis, its step or its operators must leave every digest and every counter as it was.

A case is one family on one problem with one switch setting, in a child process of its own under its own time limit (the
switches are read once per process); nothing more is started after a child fails.

* ``lanczos/membrane32`` (the 32 x 32 interior membrane pencil, 40 steps) and ``lanczos/standard400`` (no M, n = 400, 24 steps):
  the raw basis (``T``, ``V``) and one front-end solve (values, vectors: restart, Ritz vectors, row permutation).
* ``resolvent/S2k`` (n = 1953: a partial last chunk; ncv 12) and ``resolvent/S5k`` (ncv 20: three column tiles): the raw basis
  and front-end solves (gains, responses, forcings): plain, both windows, discounted at omega = 0 (real factors, complex
  vectors), ``block_forcings=True``.
* ``growth/S2k``, ``growth/S5k``: the raw basis and front-end solves for Euler and SDIRK2, with and without the response window
  (``T``, ``V``, gains, initial conditions, responses, energies).
* each of them also with ``LSA_LANCZOS_FUSED=0`` (growth: and ``LSA_GROWTH_FUSED=0``).
* ``--refine FAMILY=RTOL`` adds a case of that family on S2k with that ``ksp_rtol``, chosen between the relative residual the
  unrefined solves leave and the one the refined solves leave, so that a step is redone with the refinement step switched on.
  ``--probe`` prints both levels for the build in hand (the second from a run whose ``ksp_rtol`` no solve can meet, so that every
  solve is refined and accepted by its backward error), or the error that run ends with.

Counters per solve: the operator's ``spmv_calls``, ``sptrsv_calls``, ``refined_solves``, ``backward_accepted`` (read where the front
end reads its statistics), the handle's four counts, applies and restarts.

usage: lanczos_ab.py [OUT.json] [--refine resolvent=RTOL] [--refine growth=RTOL] [--note KEY=VALUE ...]     lanczos_ab.py --probe"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
UNFUSED = {"LSA_LANCZOS_FUSED": "0", "LSA_GROWTH_FUSED": "0"}
CASES = ("lanczos/membrane32", "lanczos/standard400", "resolvent/S2k", "resolvent/S5k", "growth/S2k", "growth/S5k")
NCV = {"S2k": 12, "S5k": 20}
DT, NSTEPS = 0.25, 4
OMEGA = 0.7379601143282424
CHILD_SECONDS = 240


def digest(a):
    import numpy as np

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class OpCounters:
    """The last operator statistics any front end read (``ShiftInvertOperator.stats``), kept for the record."""

    KEYS = ("spmv_calls", "sptrsv_calls", "refined_solves", "backward_accepted")

    def __init__(self):
        import lsa_hip

        self.seen = {}
        inner = lsa_hip.ShiftInvertOperator.stats

        def stats(op):
            d = inner(op)
            self.seen = dict(d)
            return d

        lsa_hip.ShiftInvertOperator.stats = stats

    def last(self):
        return {k: int(self.seen[k]) for k in self.KEYS} | {"max_rel_res": float(self.seen["max_rel_res"])}


def on_shared_pattern(K, M):
    import numpy as np
    import scipy.sparse as sp
    from Solver.utils import _onto_pattern

    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)  # noqa: E731
    union = (ones(K) + ones(M)).tocsr()
    union.sort_indices()
    return _onto_pattern(K, union), _onto_pattern(M, union)


def raw_basis(make_basis, A, M, sigma, ncv, v0, ksp_rtol, counters):
    """``ncv`` steps of the basis ``make_basis(ctx, op)`` builds on the operator at ``sigma``: T, V and the operator's counters."""
    import numpy as np

    import lsa_hip

    ctx = lsa_hip.Context(0)
    dA = lsa_hip.CsrMatrix.from_scipy(ctx, A)
    dM = None if M is None else lsa_hip.CsrMatrix.from_scipy(ctx, M)
    op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, sigma, mode=0, pc_type=2, ksp_rtol=ksp_rtol)
    basis = make_basis(ctx, op)
    basis.set_start(v0)
    T = np.zeros((ncv + 1, ncv), order="F")
    bd = basis.extend(0, ncv, T)
    V = basis.basis(ncv + 1)
    op.stats()
    out = {"T": digest(T), "V": digest(V), "breakdown": int(bd), "op": counters.last()}
    del basis, op, dA, dM
    ctx.close()
    return out


def lanczos_child(name, counters, _rtol):
    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType
    from synthetic import fem

    if name == "membrane32":
        A, M, bnd = fem.assemble_membrane(32, 32, 2.0, 2.0)
        keep = np.setdiff1d(np.arange(A.shape[0]), bnd)
        K, M = (sp.csr_matrix((sp.csr_matrix(X)[keep][:, keep] + sp.csr_matrix(X)[keep][:, keep].T) * 0.5) for X in (A, M))
        K.sort_indices(), M.sort_indices()
        sigma, ncv, nev, ptype, pc = 10.0, 40, 12, iEpsProblemType.GHEP, PreconditionerType.CHOLESKY
        rawK, rawM = on_shared_pattern(K, M)
    else:
        n = 400
        rng = np.random.default_rng(3)
        d, e = np.arange(1.0, n + 1.0), 0.3 * rng.standard_normal(n - 1)
        K, M = sp.diags([e, d, e], [-1, 0, 1], format="csr"), None
        sigma, ncv, nev, ptype, pc = 100.4, 24, 8, iEpsProblemType.HEP, PreconditionerType.LU
        rawK, rawM = K, None
    out = {"raw": raw_basis(lambda ctx, op: lsa_hip.LanczosBasis(ctx, op, ncv), rawK, rawM, sigma, ncv,
                            np.random.default_rng(0).standard_normal(K.shape[0]), 1e-12, counters)}
    es = EigenSolver(K, M, EigensolverConfig(num_eig=nev, problem_type=ptype, atol=1e-10, ncv=ncv), check_hermitian=False, symmetric=True)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(sigma)
    es.solver.set_st_pc_type(pc)
    es.solve()
    s = es.solver
    k = s.get_num_converged()
    out["solve"] = {"values": digest(np.array([s.get_eigenvalue(i) for i in range(k)])),
                    "vectors": digest(np.column_stack([s.get_eigenvector_array(i) for i in range(k)])), "nconv": int(k),
                    "applies": int(s.stats["op_applies"]), "restarts": int(s.stats["krylov_restarts"]), "op": counters.last()}
    return out


def cylinder(name):
    import scipy.sparse as sp
    from synthetic import fem

    es = fem.cylinder_case(name)
    return es, sp.csr_matrix(es.A), sp.csr_matrix(es.M)


def resolvent_child(name, counters, rtol):
    import numpy as np

    import lsa_hip
    from Solver.resolvent import ResolventConfig, ResolventSolver

    es, A, M = cylinder(name)
    ncv, n = NCV[name], A.shape[0]
    rng = np.random.default_rng(0)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    out = {"raw": raw_basis(lambda ctx, op: lsa_hip.ResolventBasis(ctx, op, ncv), *on_shared_pattern(A, M), 1j * OMEGA, ncv, v0,
                            rtol or 1e-12, counters)}
    x, y = es.dof_xy()
    windows = dict(forcing_window=((x >= -3) & (x <= 3) & (y >= -3) & (y <= 3)).astype(float), response_window=((x >= 2) & (x <= 30)).astype(float))
    runs = {"plain": ({}, OMEGA)} if rtol else {"plain": ({}, OMEGA), "windows": (windows, OMEGA), "discounted_omega0": ({"discount": 0.3}, 0.0),
                                                "block_forcings": ({"block_forcings": True}, OMEGA)}
    for tag, (kw, omega) in runs.items():
        rs = ResolventSolver(A, M, ResolventConfig(num_modes=4, ncv=ncv, atol=1e-10), ksp_rtol=rtol, **kw)
        res = rs.solve(omega)
        st = res.stats
        out[tag] = {"gains": digest(res.gains), "responses": digest(res.responses), "forcings": digest(res.forcings),
                    "counts": [int(st[k]) for k in ("adjoint_solves", "forward_solves", "refined_adjoint", "refined_forward")],
                    "applies": int(st["applies"]), "restarts": int(st["restarts"]), "op": counters.last()}
        rs.release()
    return out


def growth_child(name, counters, rtol):
    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    es, A, M = cylinder(name)
    ncv, n = NCV[name], A.shape[0]
    free = np.zeros(n, dtype=bool)  # the front end's rule for the constrained rows: no off-diagonal entry in A and M
    for X in (A, M):
        C = sp.coo_matrix(X)
        off = (C.row != C.col) & (C.data != 0)
        free[C.row[off]] = free[C.col[off]] = True
    v0 = np.random.default_rng(0).standard_normal(n)
    out = {}
    x, _ = es.dof_xy()
    window = ((x >= 2) & (x <= 30)).astype(float)
    for scheme in ("euler", "sdirk2"):
        sigma = 1.0 / DT if scheme == "euler" else 1.0 / ((1.0 - 1.0 / np.sqrt(2.0)) * DT)
        out[f"raw_{scheme}"] = raw_basis(lambda ctx, op: lsa_hip.GrowthBasis(ctx, op, ncv, NSTEPS, free.astype(float), scheme=scheme),
                                         *on_shared_pattern(A, M), sigma, ncv, v0, rtol or 1e-12, counters)
        for tag, kw in (("plain", {}),) if rtol else (("plain", {}), ("response_window", {"response_window": window})):
            tg = TransientGrowthSolver(A, M, TransientGrowthConfig(dt=DT, num_modes=3, ncv=ncv, atol=1e-10, scheme=scheme), ksp_rtol=rtol, **kw)
            res = tg.solve(NSTEPS * DT)
            st = res.stats
            out[f"{tag}_{scheme}"] = {"gains": digest(res.gains), "initial": digest(res.initial), "responses": digest(res.responses),
                                      "energy": digest(res.energy),
                                      "counts": [int(st[k]) for k in ("forward_solves", "transposed_solves", "refined_forward", "refined_transposed")],
                                      "applies": int(st["applies"]), "restarts": int(st["restarts"]), "op": counters.last()}
            tg.release()
        if rtol:
            break
    return out


def child(case, rtol):
    sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]
    family, name = case.split("/")
    out = {"lanczos": lanczos_child, "resolvent": resolvent_child, "growth": growth_child}[family](name, OpCounters(), rtol)
    print(json.dumps(out))


def run_child(case, env, rtol=None):
    cmd = [sys.executable, __file__, "--child", case] + ([repr(rtol)] if rtol else [])
    r = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True, timeout=CHILD_SECONDS)
    if r.returncode != 0:
        return None, (r.stdout + r.stderr)[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def probe():
    """Per family on S2k: max_rel_res of a run that did not refine, and of one in which every solve is refined."""
    out = {}
    for family in ("resolvent", "growth"):
        plain, err = run_child(f"{family}/S2k", {})
        if err:
            sys.exit(f"lanczos_ab --probe: {family} failed\n{err}")
        raw = plain["raw"] if family == "resolvent" else plain["raw_euler"]
        out[family] = {"unrefined_max_rel_res": raw["op"]["max_rel_res"], "unrefined_refined_solves": raw["op"]["refined_solves"]}
        forced, err = run_child(f"{family}/S2k", {}, 1e-30)
        if err:
            out[family]["all_refined_error"] = err.strip().splitlines()[-1]
        else:
            raw = forced["raw"] if family == "resolvent" else forced["raw_euler"]
            out[family].update(refined_max_rel_res=raw["op"]["max_rel_res"], refined_refined_solves=raw["op"]["refined_solves"],
                               refined_backward_accepted=raw["op"]["backward_accepted"])
    print(json.dumps(out, indent=1))


def main(argv):
    merged, refine, notes, path = {}, {}, {}, None
    it = iter(argv)
    for a in it:
        if a == "--refine":
            family, value = next(it).split("=")
            refine[family] = float(value)
        elif a == "--note":
            k, v = next(it).split("=", 1)
            notes[k] = v
        else:
            path = Path(a)
    runs = [(case, env, None) for case in CASES for env in ({}, UNFUSED)] + [(f"{family}/S2k", {}, rtol) for family, rtol in refine.items()]
    for case, env, rtol in runs:
        tag = f"{case} [{'unfused' if env else 'fused'}" + (f", ksp_rtol={rtol!r}]" if rtol else "]")
        got, err = run_child(case, env, rtol)
        if err:  # (nothing more is started on the GPU after a failure)
            sys.stderr.write(err)
            sys.exit(f"lanczos_ab: {tag} failed")
        merged[tag] = got
        print(tag, "done", file=sys.stderr, flush=True)
    if notes:
        merged["notes"] = notes
    text = json.dumps(merged, indent=1, sort_keys=True)
    if path:
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else None)
    elif sys.argv[1:] == ["--probe"]:
        probe()
    else:
        main(sys.argv[1:])
