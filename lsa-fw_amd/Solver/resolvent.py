"""Resolvent (input-output) analysis on the MI355X path: optimal gains, responses and forcings of ``M q' = A q + M f``.

For a real frequency ``omega`` and ``R = (i omega M - A)^-1`` the gains ``sigma_1 >= sigma_2 >= ...`` are the maxima of
``||q||_M / ||f||_M`` over ``q = R M f``: the other half of the linear analysis of a base flow, beside the eigenvalues of
:class:`Solver.eigen.EigenSolver` (same conventions: ``A x = lambda M x``).  ``sigma_j^2`` are the largest eigenvalues of
``W = R M R^H M``, self-adjoint in the ``M``-inner product; the library runs a thick-restart Lanczos iteration on it with both inner
solves of a step on ONE nested-dissection LU of ``A - i omega M`` (``lsa_resolvent_*``, ``csrc/resolvent.hip``)::

    cfg = ResolventConfig(num_modes=3, ncv=24, atol=1e-8, max_it=500)
    rs = ResolventSolver(A, M, cfg)
    res = rs.solve(0.74)                 # res.gains, res.responses, res.forcings
    curve = rs.sweep([0.2, 0.4, 0.74])   # one context, ordering and LU analysis; a refactorisation per frequency

The inner products are those of ``M`` (real symmetric positive semidefinite: a zero pressure block and identity Dirichlet rows are
fine).  Other forcing / response weights, restriction masks and lockstep over frequencies are not built.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field

import numpy as np

from .eigen import _require_matching_squares, _wrap
from .utils import PreconditionerType, iEpsProblemType, iEpsSolver, iSTType, symmetry_defect, _SYMMETRY_TOL

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class ResolventConfig:
    num_modes: int = 3  # gains (with their response and forcing modes) to compute
    ncv: int = 24  # Krylov subspace dimension
    atol: float = 1e-8  # relative tolerance on sigma^2: |beta y_mi| / theta_i
    max_it: int = 500  # restarts allowed


@dataclass
class ResolventResult:
    omega: float
    gains: np.ndarray  # sigma_j, descending
    responses: np.ndarray  # n x k complex, q_j^H M q_k = delta_jk, the entry of largest magnitude real positive
    forcings: np.ndarray | None  # n x k complex, f_j^H M f_k = delta_jk, R M f_j = sigma_j q_j (only M f_j is determined)
    estimates: np.ndarray  # relative residual estimates of sigma_j^2
    stats: dict = field(default_factory=dict)


def _real_frequency(omega) -> float:
    """``omega`` as a float; ``ValueError`` unless it is a finite real number."""
    try:
        z = complex(omega)
    except TypeError as exc:
        raise ValueError(f"omega must be a real number, got {omega!r}") from exc
    if z.imag != 0.0 or not math.isfinite(z.real):
        raise ValueError(f"omega must be a finite real frequency, got {omega!r}")
    return float(z.real)


class ResolventSolver:
    """Optimal gains of ``(A, M)`` at real frequencies; thin shell around :class:`iEpsSolver` 's preparation (union pattern,
    nested-dissection ordering, permuted numbering, upload, pattern-only LU analysis) and ``lsa_hip.ResolventBasis``."""

    def __init__(self, A, M, cfg: ResolventConfig | None = None, *, device: int = 0, layout: str = "single",
                 pc_type: PreconditionerType = PreconditionerType.LU, ilu_levels: int | None = None, seed: int = 0,
                 ksp_rtol: float | None = None, block_forcings: bool = False) -> None:
        if A is None:
            raise ValueError("Operator A is required.")
        if M is None:
            raise ValueError("Resolvent analysis needs M: the gains are measured in the M-inner product")
        A, M = _wrap(A), _wrap(M)
        _require_matching_squares(A, M)
        Ms = M.as_scipy_array()
        if Ms.dtype.kind == "c":
            raise ValueError("Resolvent analysis needs a real M (the M-inner product); M is complex")
        defect = symmetry_defect(Ms)
        if not defect <= _SYMMETRY_TOL:
            raise ValueError(f"Resolvent analysis needs a symmetric M; its relative symmetry defect is {defect:.3e}")
        self._cfg = cfg if cfg is not None else ResolventConfig()
        if self._cfg.num_modes < 1:
            raise ValueError("num_modes must be at least 1")
        if self._cfg.ncv <= self._cfg.num_modes:
            raise ValueError(f"ncv = {self._cfg.ncv} must exceed num_modes = {self._cfg.num_modes}")
        if layout != "single":
            raise NotImplementedError(f"Resolvent analysis runs on one GPU; the layout is '{layout}'")
        pc_type = PreconditionerType(pc_type)
        if pc_type not in (PreconditionerType.LU, PreconditionerType.CHOLESKY) or ilu_levels is not None:
            raise NotImplementedError("Resolvent analysis needs the exact LU (PreconditionerType.LU): both inner solves of a step run on its "
                                      f"factors; the preconditioner is {pc_type.name}" + ("" if ilu_levels is None else f" with ILU level {ilu_levels}"))
        eps = iEpsSolver(A, M, device=device, seed=seed, ksp_rtol=ksp_rtol)
        eps.set_problem_type(iEpsProblemType.GNHEP)
        eps.set_st_type(iSTType.SINVERT)
        eps.set_st_pc_type(pc_type)
        eps.set_tolerances(self._cfg.atol, self._cfg.max_it)
        eps.set_dimensions(self._cfg.num_modes, self._cfg.ncv)
        self._eps = eps
        self._seed = seed
        # the forcings' adjoint solves as one block solve on the factors (same bits; off by default)
        self._block_forcings = bool(block_forcings)

    @property
    def config(self) -> ResolventConfig:
        return self._cfg

    @property
    def solver(self) -> iEpsSolver:
        """The eigen path's solver object whose preparation this one shares (``prepare()``, ``release()``)."""
        return self._eps

    def solve(self, omega: float, forcings: bool = True) -> ResolventResult:
        """Gains, responses and (``forcings=True``) forcings at ``omega``: factorises ``A - i omega M`` (``omega = 0``: real factors)
        and iterates.  A second call on the same solver keeps the context, the ordering and the LU analysis."""
        import lsa_hip

        omega = _real_frequency(omega)
        eps, cfg = self._eps, self._cfg
        started = time.time()
        eps.set_target(complex(0.0, omega))
        run = eps._open(basis=False)
        nev, basis = run["nev"], None
        try:
            prep, op = eps._prepared, run["op"]
            if prep["pc_code"] != 2 or op.stats().get("pc_fallback"):
                raise NotImplementedError("Resolvent analysis needs the exact LU; it does not fit the device memory")
            basis = lsa_hip.ResolventBasis(prep["ctx"], op, run["ncv"])
            basis.set_row_permutation(prep["perm"])
            if self._block_forcings:
                basis.set_block_forcings(True)
            out = basis.solve(nev, cfg.atol, cfg.max_it, v0=eps._start_vector(basis.n), seed=self._seed, max_out=nev, forcings=forcings)
            st = op.stats()
            basis_bytes = basis.basis_bytes
        finally:
            del basis  # (the basis goes before its operator)
            run.clear()
        k = len(out["gains"])
        if out["nconv"] < nev:
            logger.warning("Resolvent: %d of %d gains converged in %d restarts (next estimate %.3e)", out["nconv"], nev, out["restarts"],
                           out["next_unconverged"])
        stats = {"applies": out["applies"], "restarts": out["restarts"], "nconv": out["nconv"], "adjoint_solves": out["adjoint_solves"],
                 "forward_solves": out["forward_solves"], "refinements": out["refined_adjoint"] + out["refined_forward"],
                 "refined_adjoint": out["refined_adjoint"], "refined_forward": out["refined_forward"],
                 "analysis_reused": bool(st.get("analysis_reused")), "max_rel_res": st.get("max_rel_res"), "basis_bytes": basis_bytes,
                 "seconds_factor": st.get("seconds_factor"), "seconds_solve": st.get("seconds_solve"), "seconds_expand": out["seconds_expand"],
                 "seconds_dense": out["seconds_dense"], "seconds_restart": out["seconds_restart"], "seconds_total": time.time() - started}
        return ResolventResult(omega, out["gains"], out["responses"][:, :k], out["forcings"], out["estimates"], stats)

    def sweep(self, omegas, forcings: bool = True) -> list[ResolventResult]:
        """One result per frequency on ONE context, ordering and LU analysis: every frequency after the first refactorises only
        (``stats["analysis_reused"]``), and returns the bytes a fresh solver gives for it.  (Going between ``omega = 0`` and a
        non-zero one changes the factors' scalar type and prepares anew.)"""
        omegas = [_real_frequency(w) for w in omegas]
        return [self.solve(w, forcings=forcings) for w in omegas]

    def release(self) -> None:
        self._eps.release()
