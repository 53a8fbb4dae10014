"""Transient growth on the MI355X path: optimal energy gains and initial conditions of ``M q' = A q`` over finite horizons.

The third question of a linear stability analysis, beside the eigenvalues of :class:`Solver.eigen.EigenSolver` and the gains of
:class:`Solver.resolvent.ResolventSolver` (same conventions: ``A x = lambda M x``): how much a perturbation of a *stable* flow can
grow in finite time, ``G(T) = max ||q(T)||_M^2 / ||q(0)||_M^2``, and from which initial condition.  By default time is marched by
implicit Euler: one step ``(M - dt A) q+ = M q`` is ``q+ = -sigma C^-1 M q`` with ``C = A - sigma M`` and ``sigma = 1 / dt``, the shift-invert
operator the library factorises.  Over ``N = T / dt`` steps the propagator is ``Phi = (-sigma C^-1 M)^N``, its adjoint in the
``M``-inner product is ``Phi+ = (-sigma C^-T M)^N`` on the same factors, and the gains are the largest eigenvalues of
``W = Phi+ Phi``; the library runs its thick-restart Lanczos iteration on it with a march of ``2 N`` solves on ONE nested-dissection
LU behind every step (``lsa_growth_*``, ``csrc/growth.hip``)::

    cfg = TransientGrowthConfig(dt=0.25, num_modes=2, ncv=12)
    tg = TransientGrowthSolver(A, M, cfg)
    res = tg.solve(4.0)                  # res.gains, res.initial, res.responses, res.energy, res.times
    curve = tg.sweep([2.0, 4.0, 10.0])   # one factorisation for every horizon of this dt

Constrained dofs (Dirichlet rows kept as identity rows in ``A`` and ``M``) are uncoupled scalar ODEs ``q' = q`` and no part of the
flow; unmasked, each is a spurious "gain" ``(1 - dt)^(-2 N)``.  ``constrained="auto"`` finds and leaves them out.

Implicit Euler is first order in ``dt``: at a ``dt`` of a quarter time unit its gains are a quarter low.  ``scheme="sdirk2"`` marches
by the L-stable, stiffly accurate two-stage SDIRK method with ``gamma = 1 - 1/sqrt(2)`` instead, second order in ``dt``: both stages
solve with ``M - gamma dt A``, so ``sigma = 1 / (gamma dt)`` and there is still ONE factorisation; with ``S = -sigma C^-1 M`` one time step
is ``S (a S + b I)``, ``a = 1 + sqrt(2)``, ``b = -sqrt(2)``, and every step of the iteration marches ``4 N`` solves.

The response can be measured in another weight, ``G = max ||q(T)||_Q^2 / ||q(0)||_M^2``: ``response_window=d`` (``n`` non-negative dof
weights, ``Q = D M D``: the energy inside a region, of one velocity component, ...) or ``response_weight=Q`` (a real symmetric positive
semidefinite matrix).  Only the turn of a step's march changes.  Weights on the initial condition need ``Q^-1`` and are not built, nor
are higher-order schemes and lockstep over horizons.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from .exact_lu import ExactLuFrontEnd, checked_side
from .utils import PreconditionerType

logger = logging.getLogger(__name__)

SDIRK2_GAMMA = 1.0 - 1.0 / np.sqrt(2.0)
SCHEMES = {"euler": 1.0, "sdirk2": SDIRK2_GAMMA}  # the scheme's gamma: the factorised matrix is M - gamma dt A, sigma = 1 / (gamma dt)


@dataclass(frozen=True)
class TransientGrowthConfig:
    dt: float  # the time step
    num_modes: int = 1  # gains (with their initial conditions and responses) to compute
    ncv: int = 12  # Krylov subspace dimension
    atol: float = 1e-8  # relative tolerance on G: |beta y_mi| / theta_i
    max_it: int = 500  # restarts allowed
    scheme: str = "euler"  # the time stepping: "euler" (implicit Euler, first order) or "sdirk2" (two-stage L-stable SDIRK, second order)

    def __post_init__(self):
        if self.scheme not in SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(SCHEMES)}, got {self.scheme!r}")


@dataclass
class TransientGrowthResult:
    horizon: float
    steps: int
    dt: float
    gains: np.ndarray  # G_j, descending
    initial: np.ndarray  # n x k, q0_j^T M q0_k = delta_jk, zero on constrained rows, the entry of largest magnitude positive
    responses: np.ndarray  # n x k, Phi q0_j (not normalised: its M-norm squared is G_j)
    energy: np.ndarray  # k x (steps + 1): ||Phi_s q0_j||_M^2 at s = 0..steps
    times: np.ndarray  # steps + 1: s dt
    estimates: np.ndarray  # relative residual estimates of G_j
    stats: dict = field(default_factory=dict)
    scheme: str = "euler"  # the time stepping the gains belong to (steps, dt and times count time steps, not stages)
    # k values ||Phi q0_j||_Q^2, the energy at T in the response weight (equal to gains, as ||q0_j||_M = 1); energy stays the M-energy
    response_energy: np.ndarray | None = None


def decoupled_dofs(A, M) -> np.ndarray:
    """Every index whose row *and* column hold no off-diagonal non-zero in both ``A`` and ``M``: an uncoupled scalar ODE, no part of
    the flow (sorted)."""
    n = A.shape[0]
    coupled = np.zeros(n, dtype=bool)
    for X in (A, M):
        C = sp.coo_matrix(X)
        off = (C.row != C.col) & (C.data != 0)
        coupled[C.row[off]] = True
        coupled[C.col[off]] = True
    return np.flatnonzero(~coupled)


def horizon_steps(T, dt: float) -> int:
    """``T / dt`` as a whole number of steps; ``ValueError`` unless ``T`` is a positive whole multiple of ``dt``
    (``|T / dt - round(T / dt)| <= 1e-9 T / dt``, at least one step)."""
    try:
        ratio = float(T) / dt
    except (TypeError, ValueError) as exc:
        raise ValueError(f"the horizon must be a real number, got {T!r}") from exc
    steps = round(ratio) if np.isfinite(ratio) else 0
    if not np.isfinite(ratio) or steps < 1 or abs(ratio - steps) > 1e-9 * ratio:
        raise ValueError(f"the horizon T = {T!r} is not a positive whole multiple of dt = {dt!r}")
    return int(steps)


class TransientGrowthSolver(ExactLuFrontEnd):
    """Optimal energy gains of ``(A, M)`` over horizons ``T = N dt``; thin shell around :class:`iEpsSolver` 's preparation (union
    pattern, nested-dissection ordering, permuted numbering, upload, LU) and ``lsa_hip.GrowthBasis``.  The operator and its
    factorisation of ``A - M / dt`` (``scheme="sdirk2"``: ``A - M / (gamma dt)``) are built by the first :meth:`solve` and kept until :meth:`release`."""

    NAME = "Transient growth"
    NEEDS_M = "the energy is measured in the M-inner product"
    NEEDS_LU = "every solve of the march runs on its factors"
    REAL_A = "Transient growth needs real A and M (a real march on real factors); A is complex"
    REAL_M = "Transient growth needs real A and M (a real march on real factors); M is complex"

    def __init__(self, A, M, cfg: TransientGrowthConfig, *, constrained="auto", device: int = 0, layout: str = "single",
                 pc_type: PreconditionerType = PreconditionerType.LU, ilu_levels: int | None = None, seed: int = 0,
                 ksp_rtol: float | None = None, response_window=None, response_weight=None) -> None:
        if A is not None and M is not None and cfg is None:  # (after the refusals of a missing A or M, before the pencil is looked at)
            raise ValueError("Transient growth needs a TransientGrowthConfig: the time step dt has no default")
        A, M, As, Ms = self._checked_pencil(A, M)
        # the response weight: a window (Q = D M D) or a matrix, checked here and built on the device with the basis
        self._response = checked_side("response", response_window, response_weight, Ms)
        self._cfg = cfg
        if not (np.isfinite(cfg.dt) and cfg.dt > 0.0):
            raise ValueError(f"dt = {cfg.dt!r} must be a positive time step")
        if cfg.num_modes < 1:
            raise ValueError("num_modes must be at least 1")
        if cfg.ncv <= cfg.num_modes:
            raise ValueError(f"ncv = {cfg.ncv} must exceed num_modes = {cfg.num_modes}")
        n = As.shape[0]
        if constrained is None:
            self._constrained = np.zeros(0, dtype=np.int64)
        else:
            free = decoupled_dofs(As, Ms)
            if isinstance(constrained, str):
                if constrained != "auto":
                    raise ValueError(f"constrained must be 'auto', an index array or None, got {constrained!r}")
                self._constrained = free
            else:
                idx = np.unique(np.asarray(constrained, dtype=np.int64).ravel())
                if idx.size and (idx[0] < 0 or idx[-1] >= n):
                    raise ValueError("constrained holds dof indices outside [0, n)")
                coupled = np.setdiff1d(idx, free)
                if coupled.size:
                    raise ValueError(f"constrained index {int(coupled[0])} is coupled to other dofs in A or M ({coupled.size} such indices): only a "
                                     "dof whose row and column hold no off-diagonal non-zero can be left out of the flow")
                self._constrained = idx
        self._set_up(A, M, cfg.atol, cfg.max_it, (cfg.num_modes, cfg.ncv), device=device, layout=layout, pc_type=pc_type, ilu_levels=ilu_levels,
                     seed=seed, ksp_rtol=ksp_rtol)
        self._eps.set_target(1.0 / (SCHEMES[cfg.scheme] * cfg.dt))
        self._run = None  # the operator (with its factors) and the basis, from the first solve to release()
        self._basis = None

    @property
    def config(self) -> TransientGrowthConfig:
        return self._cfg

    @property
    def constrained(self) -> np.ndarray:
        """The dof indices left out of the flow (sorted)."""
        return self._constrained

    def _open(self, steps: int):
        import lsa_hip

        run, prep = self._open_operator()
        try:
            keep = np.ones(self._n)
            keep[self._constrained] = 0.0
            basis = lsa_hip.GrowthBasis(prep["ctx"], run["op"], run["ncv"], steps, keep[prep["perm"]], self._cfg.scheme)  # (the iteration runs in permuted numbering)
            basis.set_row_permutation(prep["perm"])
            if self._response is not None:
                basis.set_response_weight(*self._weights_on_device(prep, (self._response,)))
        except BaseException:
            run.clear()
            raise
        self._run, self._basis = run, basis

    def solve(self, T: float) -> TransientGrowthResult:
        """Gains, initial conditions, responses and energy curves at the horizon ``T``, a positive whole multiple of ``dt``.  The first
        call orders, analyses and factorises ``A - sigma M``; every later one changes the number of steps only and returns the bytes a
        fresh solver gives for its horizon."""
        cfg = self._cfg
        steps = horizon_steps(T, cfg.dt)
        started = time.time()
        reused = self._basis is not None
        if reused:
            self._basis.set_steps(steps)
        else:
            self._open(steps)
        run, basis = self._run, self._basis
        nev, op = run["nev"], run["op"]
        before = op.stats()
        rng = np.random.default_rng(self._seed)
        out = basis.solve(nev, cfg.atol, cfg.max_it, v0=rng.standard_normal(basis.n), seed=self._seed, max_out=nev)
        st = op.stats()
        k = len(out["gains"])
        if out["nconv"] < nev:
            logger.warning("Transient growth: %d of %d gains converged in %d restarts (next estimate %.3e)", out["nconv"], nev, out["restarts"],
                           out["next_unconverged"])
        stats = {"applies": out["applies"], "restarts": out["restarts"], "nconv": out["nconv"], "forward_solves": out["forward_solves"],
                 "transposed_solves": out["transposed_solves"], "refinements": out["refined_forward"] + out["refined_transposed"],
                 "refined_forward": out["refined_forward"], "refined_transposed": out["refined_transposed"], "factorisation_reused": reused,
                 "constrained": int(self._constrained.size), "spmv_calls": st.get("spmv_calls"), "max_rel_res": st.get("max_rel_res"), "basis_bytes": basis.basis_bytes,
                 "seconds_factor": st.get("seconds_factor"), "seconds_solve": st.get("seconds_solve") - (before.get("seconds_solve") if reused else 0.0),
                 "seconds_expand": out["seconds_expand"], "seconds_dense": out["seconds_dense"], "seconds_restart": out["seconds_restart"],
                 "seconds_total": time.time() - started}
        return TransientGrowthResult(float(T), steps, cfg.dt, out["gains"], out["initial"][:, :k], out["responses"][:, :k], out["energy"][:k],
                                     cfg.dt * np.arange(steps + 1), out["estimates"], stats, cfg.scheme, out["response_energy"])

    def sweep(self, horizons) -> list[TransientGrowthResult]:
        """One result per horizon on ONE factorisation: every horizon after the first changes the number of steps only
        (``stats["factorisation_reused"]``) and returns the bytes a fresh solver gives for it."""
        for T in horizons:
            horizon_steps(T, self._cfg.dt)  # (a bad horizon is refused before the first one runs)
        return [self.solve(T) for T in horizons]

    def release(self) -> None:
        self._basis = None  # (the basis goes before its operator)
        if self._run is not None:
            self._run.clear()
            self._run = None
        super().release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
