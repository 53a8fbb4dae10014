"""What the analyses on the exact LU of a pencil ``(A, M)`` share: :class:`Solver.resolvent.ResolventSolver`,
:class:`Solver.growth.TransientGrowthSolver`, :class:`Solver.stochastic.StochasticForcingSolver` and
:class:`Solver.region.RegionEigenSolver`.  Each is a thin shell around :class:`iEpsSolver` 's preparation (union pattern,
nested-dissection ordering, permuted numbering, upload, pattern-only LU analysis) and a handle of ``lsa_hip`` that iterates on the
factors.  :class:`ExactLuFrontEnd` holds the constructor's checks of the pencil and of the layout and preconditioner, the set-up of
the ``iEpsSolver``, "prepare at this shift and insist on the exact LU", and the weights on the device; the checks of windows and
weights that resolvent, growth and stochastic forcing share live here too.  A front end talks to its ``iEpsSolver`` through public
names only.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .eigen import _require_matching_squares, _wrap
from .utils import PreconditionerType, iEpsProblemType, iEpsSolver, iSTType, symmetry_defect, _onto_pattern, _permute, _SYMMETRY_TOL


def checked_window(name: str, window, Ms) -> np.ndarray:
    """The window ``name`` as ``n`` float64 dof weights; ``ValueError`` unless it is a real array of ``n`` non-negative finite entries
    under which ``D M D`` keeps a positive diagonal entry (some mass inside).  Pure host work."""
    n = Ms.shape[0]
    d = np.asarray(window)
    if d.dtype.kind == "c":
        raise ValueError(f"{name} has complex entries: a window is a real array of non-negative dof weights")
    if d.dtype.kind not in "fiub":
        raise ValueError(f"{name} must be a real array of dof weights, got dtype {d.dtype}")
    if d.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {d.shape}")
    d = np.ascontiguousarray(d, dtype=np.float64)
    if not np.isfinite(d).all():
        raise ValueError(f"{name} has NaN or infinite entries")
    if (d < 0.0).any():
        raise ValueError(f"{name} has negative entries: a window is non-negative")
    if not ((d * Ms.diagonal()) * d > 0.0).any():
        raise ValueError(f"{name} leaves no mass inside: D M D has no positive diagonal entry")
    return d


def checked_weight(name: str, weight, n: int):
    """The weight ``name`` as a float64 CSR matrix; ``ValueError`` unless it is real, ``n x n``, finite and symmetric (the rule ``M``
    is held to).  Pure host work."""
    Q = _wrap(weight).as_scipy_array()
    if Q.shape != (n, n):
        raise ValueError(f"{name} must have shape ({n}, {n}), got {Q.shape}")
    if Q.dtype.kind == "c":
        raise ValueError(f"{name} is complex: a weight is a real symmetric positive semidefinite matrix")
    Q = sp.csr_matrix(Q, dtype=np.float64)
    Q.sum_duplicates()  # (also sorts the indices: one entry per position, as the upload wants them)
    if not np.isfinite(Q.data).all():
        raise ValueError(f"{name} has NaN or infinite entries")
    defect = symmetry_defect(Q)
    if not defect <= _SYMMETRY_TOL:
        raise ValueError(f"{name} must be symmetric; its relative symmetry defect is {defect:.3e}")
    return Q


def checked_side(side: str, window, weight, Ms):
    """One side's weighting as given to a front end: ``None`` (``M``), ``("window", d)`` or ``("weight", Q)``; a window and a weight
    for the same side is a ``ValueError``."""
    if window is not None and weight is not None:
        raise ValueError(f"{side}_window and {side}_weight are both given: one side takes a window or a weight, not both")
    if window is not None:
        return "window", checked_window(f"{side}_window", window, Ms)
    if weight is not None:
        return "weight", checked_weight(f"{side}_weight", weight, Ms.shape[0])
    return None


def shared_pattern(A, M):
    """The pattern the prepared device pair ``(A, M)`` stands on, as a CSR matrix of ones: the union of both (``iEpsSolver.prepare``)."""
    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)  # noqa: E731
    union = (ones(sp.csr_matrix(A)) + ones(sp.csr_matrix(M))).tocsr()
    union.sort_indices()
    return union


def device_weight(prep: dict, spec, pattern=None):
    """The device matrix of a checked side on the prepared, permuted numbering: ``D M D`` by ``CsrMatrix.windowed`` on the prepared
    ``M`` for a window, an upload of the permuted matrix for a weight, ``None`` for ``M`` itself.  A weight whose entries all lie on
    ``pattern`` (:func:`shared_pattern`) is uploaded on that pattern, explicit zeros included: its products then run in the kernel form
    and summation order of ``M``'s, and ``weight = M`` gives the bits of no weight."""
    import lsa_hip

    if spec is None:
        return None
    kind, what = spec
    perm = prep["perm"]
    if kind == "window":
        return prep["dM"].windowed(what[perm])
    if pattern is not None:
        mine = sp.csr_matrix((np.ones(what.nnz), what.indices, what.indptr), shape=what.shape)
        if (pattern + mine).nnz == pattern.nnz:
            what = _onto_pattern(what, pattern)
    return lsa_hip.CsrMatrix.from_scipy(prep["ctx"], _permute(what, perm))


class ExactLuFrontEnd:
    """An analysis on the exact LU of ``(A, M)``, one GPU.  A subclass supplies the texts below and calls, from its constructor,
    :meth:`_checked_pencil`, then its own checks, then :meth:`_set_up` (the order in which two broken rules are reported is part of
    the behaviour); its solves begin with :meth:`_prepare` or :meth:`_open_operator`."""

    NAME = ""  # the front end as its messages name it ("Resolvent analysis")
    NEEDS_M = ""  # why M is required ("the gains are measured in the M-inner product")
    NEEDS_LU = ""  # why the exact LU is required ("both inner solves of a step run on its factors")
    REAL_A: str | None = None  # the refusal of a complex A (``None``: a complex A is fine)
    REAL_M = ""  # the refusal of a complex M
    SYMMETRIC_M = True  # M is held to ``_SYMMETRY_TOL``

    def _checked_pencil(self, A, M):
        """``(A, M, As, Ms)``, wrapped and as scipy matrices, behind the checks of the pair: both given, square and of one shape, real
        where the analysis needs it, ``M`` symmetric."""
        if A is None:
            raise ValueError("Operator A is required.")
        if M is None:
            raise ValueError(f"{self.NAME} needs M: {self.NEEDS_M}")
        A, M = _wrap(A), _wrap(M)
        _require_matching_squares(A, M)
        As, Ms = A.as_scipy_array(), M.as_scipy_array()
        if self.REAL_A is not None and As.dtype.kind == "c":
            raise ValueError(self.REAL_A)
        if Ms.dtype.kind == "c":
            raise ValueError(self.REAL_M)
        if self.SYMMETRIC_M:
            defect = symmetry_defect(Ms)
            if not defect <= _SYMMETRY_TOL:
                raise ValueError(f"{self.NAME} needs a symmetric M; its relative symmetry defect is {defect:.3e}")
        return A, M, As, Ms

    def _set_up(self, A, M, atol: float, max_it: int, dimensions, *, device, layout, pc_type, ilu_levels, seed, ksp_rtol) -> None:
        """The checks of layout and preconditioner, then the ``iEpsSolver`` whose preparation this analysis shares: shift-invert on
        ``pc_type``, the tolerances, and ``dimensions = (nev, ncv)`` where the analysis iterates on a Krylov basis (``None``: not set)."""
        if layout != "single":
            raise NotImplementedError(f"{self.NAME} runs on one GPU; the layout is '{layout}'")
        pc_type = PreconditionerType(pc_type)
        if pc_type not in (PreconditionerType.LU, PreconditionerType.CHOLESKY) or ilu_levels is not None:
            raise NotImplementedError(f"{self.NAME} needs the exact LU (PreconditionerType.LU): {self.NEEDS_LU}; the preconditioner is "
                                      f"{pc_type.name}" + ("" if ilu_levels is None else f" with ILU level {ilu_levels}"))
        eps = iEpsSolver(A, M, device=device, seed=seed, ksp_rtol=ksp_rtol)
        eps.set_problem_type(iEpsProblemType.GNHEP)
        eps.set_st_type(iSTType.SINVERT)
        eps.set_st_pc_type(pc_type)
        eps.set_tolerances(atol, max_it)
        if dimensions is not None:
            eps.set_dimensions(*dimensions)
        self._eps = eps
        self._n = A.shape[0]
        self._seed = seed
        # the inner solves' tolerance a handle that factorises for itself is given
        self._ksp_rtol = ksp_rtol if ksp_rtol is not None else float(np.clip(atol * 1e-2, 1e-13, 1e-8))

    @property
    def solver(self) -> iEpsSolver:
        """The eigen path's solver object whose preparation this one shares (``prepare()``, ``release()``)."""
        return self._eps

    def _prepare(self, shift: complex):
        """Prepare at ``shift`` and insist on the exact LU: ``(prep, ctx, perm)`` of the preparation."""
        self._eps.set_target(shift)
        self._eps.prepare()
        prep = self._eps.prepared
        if prep["pc_code"] != 2:
            raise NotImplementedError(f"{self.NAME} needs the exact LU")
        return prep, prep["ctx"], prep["perm"]

    def _open_operator(self, shift: complex | None = None):
        """``(run, prep)``: the operator built and factorised at ``shift`` (``None``: the target as it stands), which must be the
        exact LU and must not have fallen back; the caller clears ``run``."""
        if shift is not None:
            self._eps.set_target(shift)
        run = self._eps.open_operator()
        try:
            prep = self._eps.prepared
            if prep["pc_code"] != 2 or run["op"].stats().get("pc_fallback"):
                raise NotImplementedError(f"{self.NAME} needs the exact LU; it does not fit the device memory")
        except BaseException:
            run.clear()
            raise
        return run, prep

    def _weights_on_device(self, prep: dict, sides, key: str | None = None) -> tuple:
        """The checked ``sides`` as device matrices (``None``: ``M``); with ``key`` built once per preparation and kept with it."""
        built = prep.get(key) if key else None
        if built is None:
            A, M = self._eps.operators
            needs = any(spec is not None and spec[0] == "weight" for spec in sides)
            pattern = shared_pattern(A.as_scipy_array(), M.as_scipy_array()) if needs else None
            built = tuple(device_weight(prep, spec, pattern) for spec in sides)
            if key:
                prep[key] = built
        return built

    def release(self) -> None:
        self._eps.release()
