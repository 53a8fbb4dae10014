"""Front end of the MI355X eigen path with the public surface of the reference's ``Solver/eigen.py``.

What callers see is unchanged -- ``EigensolverConfig``, ``EigenSolver(A, M, cfg, *, check_hermitian)``, the ``solver`` and
``config`` properties, ``solve()`` returning ``[(eigenvalue, iComplexPETScVector), ...]`` -- so the reference's own usage
example (``Solver/eigen.py:6-23``) runs as written::

    cfg = EigensolverConfig(num_eig=6, problem_type=iEpsProblemType.GNHEP, atol=1e-8, max_it=500)
    es = EigenSolver(A, M, cfg)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(0.018 + 0.738j)
    es.solver.set_st_pc_type(PreconditionerType.ILU)
    eigenpairs = es.solve()

Everything numerical happens behind ``es.solver`` (:class:`Solver.utils.iEpsSolver`, HIP kernels through
``liblsa_hip.so``).  Two call orders are understood, told apart by argument type: the current one and the older
``EigenSolver(cfg, A=..., M=...)`` that the reference's tests, CLI and docs still use
(``tests/unit/Solver/test_eigen.py:91``, ``Solver/cli.py:168``).
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass

from FEM.utils import iComplexPETScVector, iPETScMatrix

from .utils import iEpsProblemType, iEpsSolver

logger = logging.getLogger(__name__)

# problem types for which SLEPc assumes a Hermitian A (and, for the generalized ones, a Hermitian M)
_NEEDS_HERMITIAN_A = frozenset({iEpsProblemType.HEP, iEpsProblemType.GHEP, iEpsProblemType.GHIEP})
_NEEDS_HERMITIAN_M = frozenset({iEpsProblemType.GHEP, iEpsProblemType.GHIEP})


@dataclass(frozen=True)
class EigensolverConfig:
    """The five knobs of ``Solver/eigen.py:48-61``, same names and defaults."""

    num_eig: int = 5  # eigenpairs to compute
    problem_type: iEpsProblemType = iEpsProblemType.GNHEP
    atol: float = 1e-6  # tolerance of the relative convergence test (EPS_CONV_REL)
    max_it: int = 500  # restarts allowed
    ncv: int = 80  # Krylov subspace dimension


def _wrap(operator):
    """Anything with a CSR view (reference wrapper, scipy matrix, ndarray) as the local matrix shim."""
    return operator if isinstance(operator, iPETScMatrix) else iPETScMatrix.from_matrix(operator)


def _sort_arguments(args, kwargs):
    """(A, M, cfg) from positional arguments in either call order plus the ``A=``, ``M=``, ``cfg=`` keywords."""
    A, M, cfg = kwargs.pop("A", None), kwargs.pop("M", None), kwargs.pop("cfg", None)
    for item in args:
        if isinstance(item, EigensolverConfig):
            cfg = item
        elif A is None:
            A = item
        elif M is None:
            M = item
        else:
            raise TypeError("EigenSolver takes at most the operators A, M and one EigensolverConfig")
    return A, M, cfg


def _require_matching_squares(A: iPETScMatrix, M: iPETScMatrix | None) -> None:
    """``ValueError`` for a non-square A or an M of another shape (``Solver/eigen.py:78-87``)."""
    rows, cols = A.shape
    if rows != cols:
        raise ValueError(f"Operator A must be square, got shape ({rows}, {cols})")
    if M is not None and tuple(M.shape) != (rows, cols):
        raise ValueError(f"Operator M shape {M.shape} does not match A's shape {A.shape}")


def _warn_about_symmetry(kind: iEpsProblemType, A: iPETScMatrix, M: iPETScMatrix | None) -> None:
    """The reference's advisory check (``:88-108``): a Hermitian problem type with a numerically non-Hermitian operator
    only earns a warning.  (There the M branch reads the *argument* ``cfg``, ``None`` when defaulted -- ``:106``; here the
    effective configuration is used.)"""
    message = "Problem type '%s' assumes Hermitian %s, but %s is not (numerically) Hermitian."
    if kind in _NEEDS_HERMITIAN_A and not A.is_numerically_hermitian():
        logger.warning(message, kind.name, "A", "A")
    if M is not None and kind in _NEEDS_HERMITIAN_M and not M.is_numerically_hermitian():
        logger.warning(message, kind.name, "M", "M")


class EigenSolver:
    """``A x = lambda M x`` (``M`` optional) on the GPU; thin shell around :class:`iEpsSolver`."""

    def __init__(self, *args, check_hermitian: bool = True, symmetric: bool = False, two_sided: bool = False, **solver_kwargs) -> None:
        """``EigenSolver(A, M=None, cfg=None, *, check_hermitian=True)`` as in ``Solver/eigen.py:67-74``, or the legacy
        ``EigenSolver(cfg, A=..., M=...)``.  Keywords the reference does not know (``device``, ``ilu_levels``,
        ``restart``, ``layout``, ...) are handed to :class:`iEpsSolver`.

        ``symmetric=True`` (build-only, default off): ``HEP`` / ``GHEP`` problems with real symmetric operators, shift-invert at
        a real target and the exact factorisation run the real thick-restart Lanczos iteration in the ``M``-inner product
        (what SLEPc does for ``GHEP``): eigenvalues are ``float``, eigenvectors real with ``x^T M x = 1``.  Anything else runs
        the general iteration as before and says why in ``solver.stats["symmetric_fallback"]``.

        ``two_sided=True`` (build-only, default off): the solve also computes the left eigenvectors ``a^H A = lambda a^H M`` on the
        factorisation it has (:meth:`iEpsSolver.set_two_sided`); :meth:`solve` returns what it returns without it,
        :meth:`left_eigenvectors` the left vectors, ``solver.get_condition_numbers()`` the condition numbers of the eigenvalues."""
        A, M, cfg = _sort_arguments(args, solver_kwargs)
        if A is None:
            raise ValueError("Operator A is required.")
        A = _wrap(A)
        M = None if M is None else _wrap(M)
        _require_matching_squares(A, M)
        self._cfg = cfg if cfg is not None else EigensolverConfig()
        if check_hermitian:
            _warn_about_symmetry(self._cfg.problem_type, A, M)

        eps = iEpsSolver(A, M, symmetric=symmetric, two_sided=two_sided, **solver_kwargs)
        eps.set_problem_type(self._cfg.problem_type)
        eps.set_tolerances(self._cfg.atol, self._cfg.max_it)
        eps.set_dimensions(self._cfg.num_eig, self._cfg.ncv)
        self._solver = eps

    @property
    def solver(self) -> iEpsSolver:
        """The configurable solver object (``set_st_type``, ``set_target``, ``set_st_pc_type``, ...)."""
        return self._solver

    @property
    def config(self) -> EigensolverConfig:
        """The configuration this solver was built with."""
        return self._cfg

    def solve(self) -> list[tuple[float | complex, iComplexPETScVector]]:
        """Solve and hand back up to ``num_eig`` converged pairs, wanted first (``Solver/eigen.py:125-155``)."""
        cfg = self._cfg
        logger.info("Started eigenvalue solve: type=%s, nev=%d, tol=%g, max_it=%d", cfg.problem_type.name, cfg.num_eig, cfg.atol, cfg.max_it)
        started = time.time()
        self._solver.solve()
        seconds = time.time() - started
        inner = self._solver.stats.get("gmres_iters")
        logger.info("Solve completed in %.2f s; converged %d eigenpairs%s", seconds, self._solver.get_num_converged(),
                    "" if inner is None else f"; iterations={inner}")
        return self._pairs()

    def _pairs(self) -> list[tuple[float | complex, iComplexPETScVector]]:
        """What :meth:`solve` hands back, from the solver's collected results."""
        pairs = list(self._solver.get_all_eigenpairs_up_to(self._cfg.num_eig))
        logger.info("Retrieved %d eigenpairs", len(pairs))
        return pairs


    def left_eigenvectors(self, normalise: str = "biorth") -> list[iComplexPETScVector | None]:
        """The left eigenvectors of the last two-sided solve, aligned with the pairs :meth:`solve` returned (``None`` where a pair
        found no left partner); ``normalise="biorth"``: ``a_i^H M v_i = 1``, ``"unit"``: 2-norm 1.

        ``v_i`` there is the stored eigenvector, ``solver.get_eigenvector_array(i)``.  :meth:`solve` hands out the same vector except
        where its imaginary part has a norm <= 1e-6: then it returns the renormalised real part (as the reference's real build
        does), and ``a_i^H M v_i = 1`` holds with THAT vector only to about 1e-6."""
        count = min(self._solver.get_num_converged(), self._cfg.num_eig)
        return [self._solver.get_left_eigenvector(i, normalise) for i in range(count)]


def _solve_group_in_turn(solvers, group, results) -> None:
    """The members of a prepared group one after another on the group's context (each its own factorisation and iteration)."""
    prev = None
    for i in group:
        eps = solvers[i].solver
        if prev is not None and prev.stats.get("analysis_reused") != 1:
            # the previous factorisation did not run on the group's analysis: the context holds another one now
            eps.redo_pattern_phase()
        results[i] = solvers[i].solve()
        eps._stats.update({"shared_analysis": True, "batch_size": len(group)})
        prev = eps


def _solve_group_lockstep(solvers, group, results, max_batch: int) -> None:
    """The members of a prepared group with all their operators and Krylov workspaces alive at once and ONE
    ``lsa_krylov_solve_batch`` over them; as many at a time (a chunk) as 0.8 of the free device memory holds.  The library decides
    per problem and expansion whether its steps can run in lockstep and runs them through the solo code otherwise; only a member
    that cannot enter the call at all (the symmetric iteration, the Python test double of the outer loop) or whose factorisation
    analysed again runs its own iteration after the chunk's call.  A member that fails does not stop the others of its chunk:
    its error is raised once they are collected."""
    import lsa_hip

    from .batch import plan_batches
    from .utils import _native_driver

    lead = solvers[group[0]].solver
    try:
        per_problem = lead.lockstep_bytes_per_problem()
    except ValueError:  # (no prepared analysis: the exact LU did not fit; the in-turn path answers that as .solve() does)
        per_problem = 0
    free, _total = lead._prepared["ctx"].mem_info()
    sub = plan_batches([solvers[i].solver for i in group], max_batch, bytes_per_problem=per_problem, memory_budget=int(0.8 * free))
    chunks = [[group[q] for q in c] for c in sub.groups]
    if per_problem == 0 or (len(group) > 1 and all(len(c) == 1 for c in chunks)):  # the budget cuts the group to one problem at a time
        logger.info("Lockstep: device memory holds one problem of this group at a time; solving one after another")
        _solve_group_in_turn(solvers, group, results)
        return
    failed: list[BaseException] = []
    for chunk in chunks:
        runs: list[dict] = []
        try:
            for i in chunk:
                eps = solvers[i].solver
                if i != group[0]:
                    # The prepared analysis went into an earlier member's factorisation (alive, or parked with another analysis
                    # if it analysed again): the pattern-only phase runs again from the shared forest, so that this member
                    # factorises on the analysis of its solo solve -- the group's.
                    eps.redo_pattern_phase()
                run = eps._open()
                runs.append(run)
                reused = run["op"].stats().get("analysis_reused") == 1
                run["eligible"] = bool(_native_driver() and reused and not run["use_lanczos"] and run["basis"] is not None and run["mask"] is None)
            members = [q for q, run in enumerate(runs) if run["eligible"]]
            errors: dict[int, BaseException] = {}
            if members:
                args = [solvers[chunk[q]].solver._native_krylov_arguments(runs[q]) for q in members]
                first = args[0]
                res, info = lsa_hip.KrylovBasis.solve_batch(
                    [runs[q]["basis"] for q in members], first["nev"], first["tol"], first["max_restarts"], first["which"], first["transform"],
                    [a["sigma"] for a in args], antishift=[a["antishift"] for a in args], targets=[a["target"] for a in args], v0s=first["v0"],
                    seed=first["seed"], raise_on_error=False)
                logger.info("Lockstep group of %d: %d rounds, %.1f launches per round, %d read-backs", len(members), info["rounds"],
                            info["launches_per_round"], info["periods"])
                for z, q in enumerate(members):
                    if isinstance(res[z], BaseException):
                        errors[q] = res[z]
                        continue
                    runs[q]["res"] = res[z]
                    runs[q]["lockstep"] = {"lockstep": info["lockstep_steps"][z] > 0, "lockstep_steps": info["lockstep_steps"][z],
                                           "solo_steps": info["solo_steps"][z], "lockstep_rounds": info["rounds"],
                                           "lockstep_launches_per_round": info["launches_per_round"]}
            for q, i in enumerate(chunk):
                if q in errors:
                    continue
                eps = solvers[i].solver
                if runs[q]["res"] is None:
                    eps._run(runs[q])
                    runs[q]["lockstep"] = {"lockstep": False, "lockstep_steps": 0, "solo_steps": int(runs[q]["res"].op_applies)}
                eps._collect(runs[q])
                eps._stats.update({"shared_analysis": True, "batch_size": len(group)})
                results[i] = solvers[i]._pairs()
            failed.extend(errors[q] for q in sorted(errors))
        finally:
            for run in runs:
                run.clear()
    if failed:
        raise failed[0]


def solve_batch(solvers, *, max_batch: int = 8, lockstep: bool = False) -> list[list[tuple[float | complex, iComplexPETScVector]]]:
    """Solve several :class:`EigenSolver` s built as for ``.solve()`` (a parameter sweep on one mesh) and return what each
    ``.solve()`` returns, in order.  Every solver is left as ``.solve()`` leaves it (``get_eigenvalue``,
    ``get_eigenvector``, ``residuals()``, ``stats``).

    Solvers with one sparsity pattern and one configuration apart from the target (shift-invert with the exact LU, one
    GPU, forward problem, no projection, the same real or complex factor type: :func:`Solver.batch.plan_batches`) form
    groups of at most ``max_batch``: a group shares one context, one fill-reducing ordering, one pattern-only analysis of
    the LU and its index tables (pattern-keyed reuse); each problem then runs its own numeric factorisation and
    Krylov-Schur iteration, one problem after another, and returns exactly the bits of a solo solve.
    ``stats["shared_analysis"]`` says whether a solver took the group path (``stats["batch_size"]``: its group's size);
    every other solver is solved alone (one log line says why).

    ``lockstep=True`` (build-only, default off): a group factorises all its problems first -- as many factor sets and Krylov
    workspaces alive at once as 0.8 of the free device memory holds -- and runs ONE ``lsa_krylov_solve_batch`` over them:
    every Arnoldi round queues one step of each problem as one batched sweep pair and one batched reduction, update and tail
    launch, one read-back covers up to 16 rounds of all problems; Schur forms and restarts stay per problem.  Still the bits of
    a solo solve.  ``stats["lockstep"]`` says whether a solver's steps ran that way, ``stats["lockstep_steps"]`` and
    ``stats["solo_steps"]`` how many did and did not."""
    from .batch import plan_batches
    from .utils import SharedContext

    if not isinstance(lockstep, bool):
        raise TypeError(f"lockstep must be a bool, got {type(lockstep).__name__}")
    solvers = list(solvers)
    if not solvers:
        raise ValueError("solve_batch needs at least one solver")
    for s in solvers:
        if not isinstance(s, EigenSolver):
            raise TypeError(f"solve_batch takes EigenSolver objects, got {type(s).__name__}")
    if len({id(s) for s in solvers}) != len(solvers):
        raise ValueError("solve_batch: a solver appears more than once")
    plan = plan_batches([s.solver for s in solvers], max_batch)
    results: list = [None] * len(solvers)
    for group in plan.groups:
        lead = solvers[group[0]].solver
        lead.prepare()
        prep = lead._prepared
        if prep.get("share") is None:
            prep["share"] = SharedContext()
        for i in group[1:]:
            solvers[i].solver.prepare(_share=prep)
        logger.info("Group of %d eigenproblems on one pattern: one context, ordering and LU analysis", len(group))
        if lockstep:
            _solve_group_lockstep(solvers, group, results, max_batch)
        else:
            _solve_group_in_turn(solvers, group, results)
    for i, reason in sorted(plan.alone.items()):
        logger.info("Eigenproblem %d is solved alone: %s", i, reason)
        results[i] = solvers[i].solve()
        solvers[i].solver._stats.update({"shared_analysis": False, "batch_size": 1})
    return results
