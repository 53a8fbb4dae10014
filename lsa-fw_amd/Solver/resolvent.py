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

By default the inner products are those of ``M`` (real symmetric positive semidefinite: a zero pressure block and identity
Dirichlet rows are fine).  Forcing and response can be weighted separately, ``sigma = max ||q||_Qq / ||f||_Qf`` over ``q = R Qf f``::

    inside = (x >= -3) & (x <= 3)                                  # a window: n non-negative dof weights, 0/1 or smooth
    rs = ResolventSolver(A, M, cfg, forcing_window=inside, response_window=(x >= 2).astype(float))   # Q = D M D
    rs = ResolventSolver(A, M, cfg, response_weight=Q)             # or any real symmetric positive semidefinite matrix

``discount=beta`` shifts to ``((beta + i omega) M - A)^-1``, the discounted resolvent for an unstable base flow (``beta`` above the
largest growth rate), and :meth:`ResolventSolver.norm_map` returns ``sigma_1(z)`` over complex points ``z``: ``1 / sigma_1`` is the
epsilon-level of the energy-norm pseudospectrum.  ``sweep(omegas, lockstep=True)`` and ``norm_map(points, warm_start=False,
lockstep=True)`` advance up to 16 frequencies or points together, one batched launch per launch of a solo step, with the bytes of
the default.  Windows that project the operator, complex Hermitian weights and several ranks are not built.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field

import numpy as np

from .exact_lu import ExactLuFrontEnd, checked_side, checked_weight, checked_window, device_weight, shared_pattern  # noqa: F401  (re-exported)
from .utils import PreconditionerType

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class ResolventConfig:
    num_modes: int = 3  # gains (with their response and forcing modes) to compute
    ncv: int = 24  # Krylov subspace dimension
    atol: float = 1e-8  # relative tolerance on sigma^2: |beta y_mi| / theta_i
    max_it: int = 500  # restarts allowed


@dataclass
class ResolventResult:
    """``Qq`` and ``Qf`` below are the response and forcing weights of the solver (``D M D`` for a window ``D``); both are ``M``
    where none was given."""

    omega: float
    gains: np.ndarray  # sigma_j = ||q_j||_Qq / ||f_j||_Qf, descending
    responses: np.ndarray  # n x k complex, q_j^H Qq q_k = delta_jk, the entry of largest magnitude real positive
    forcings: np.ndarray | None  # n x k complex, f_j^H Qf f_k = delta_jk, R Qf f_j = sigma_j q_j (only Qf f_j is determined)
    estimates: np.ndarray  # relative residual estimates of sigma_j^2
    stats: dict = field(default_factory=dict)
    discount: float = 0.0  # beta of the shift beta + i omega: R = ((beta + i omega) M - A)^-1


def _real_frequency(omega) -> float:
    """``omega`` as a float; ``ValueError`` unless it is a finite real number."""
    try:
        z = complex(omega)
    except TypeError as exc:
        raise ValueError(f"omega must be a real number, got {omega!r}") from exc
    if z.imag != 0.0 or not math.isfinite(z.real):
        raise ValueError(f"omega must be a finite real frequency, got {omega!r}")
    return float(z.real)


def _real_discount(beta) -> float:
    """``beta`` as a float; ``ValueError`` unless it is a finite real number."""
    try:
        z = complex(beta)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"discount must be a real number, got {beta!r}") from exc
    if z.imag != 0.0 or not math.isfinite(z.real):
        raise ValueError(f"discount must be a finite real number, got {beta!r}")
    return float(z.real)


class ResolventSolver(ExactLuFrontEnd):
    """Optimal gains of ``(A, M)`` at real frequencies (``discount``: at ``beta + i omega``), with optional forcing and response
    windows or weights; thin shell around :class:`iEpsSolver` 's preparation (union pattern,
    nested-dissection ordering, permuted numbering, upload, pattern-only LU analysis) and ``lsa_hip.ResolventBasis``."""

    NAME = "Resolvent analysis"
    NEEDS_M = "the gains are measured in the M-inner product"
    NEEDS_LU = "both inner solves of a step run on its factors"
    REAL_M = "Resolvent analysis needs a real M (the M-inner product); M is complex"

    def __init__(self, A, M, cfg: ResolventConfig | None = None, *, device: int = 0, layout: str = "single",
                 pc_type: PreconditionerType = PreconditionerType.LU, ilu_levels: int | None = None, seed: int = 0,
                 ksp_rtol: float | None = None, block_forcings: bool = False, forcing_window=None, response_window=None,
                 forcing_weight=None, response_weight=None, discount: float = 0.0) -> None:
        A, M, _, Ms = self._checked_pencil(A, M)
        # forcing and response weights: a window D (n non-negative dof weights in the caller's numbering: Q = D M D) or a real
        # symmetric positive semidefinite matrix per side; checked here, built on the device once per preparation
        self._sides = (checked_side("forcing", forcing_window, forcing_weight, Ms), checked_side("response", response_window, response_weight, Ms))
        self._discount = _real_discount(discount)
        self.last_map_stats: list[dict] = []
        self.last_lockstep_info: list[dict] = []  # the counters of every group call of the last lockstep sweep or map
        self._cfg = cfg = cfg if cfg is not None else ResolventConfig()
        if cfg.num_modes < 1:
            raise ValueError("num_modes must be at least 1")
        if cfg.ncv <= cfg.num_modes:
            raise ValueError(f"ncv = {cfg.ncv} must exceed num_modes = {cfg.num_modes}")
        self._set_up(A, M, cfg.atol, cfg.max_it, (cfg.num_modes, cfg.ncv), device=device, layout=layout, pc_type=pc_type, ilu_levels=ilu_levels,
                     seed=seed, ksp_rtol=ksp_rtol)
        # the forcings' adjoint solves as one block solve on the factors (same bits; off by default)
        self._block_forcings = bool(block_forcings)

    @property
    def config(self) -> ResolventConfig:
        return self._cfg

    def _iterate(self, shift: complex, nev: int, forcings: bool, warm=None):
        """The iteration at one complex shift: factorises ``A - shift M`` (a real shift: real factors) and runs ``nev`` modes.
        ``warm``: a start vector in the caller's numbering instead of the default one.  Returns the library's output and the
        statistics of the solve."""
        import lsa_hip

        eps, cfg = self._eps, self._cfg
        started = time.time()
        before = eps.prepared
        run, prep = self._open_operator(shift)
        basis = None
        try:
            op = run["op"]
            prepared_anew = prep is not before  # (the first solve, or a change between real and complex factors)
            basis = lsa_hip.ResolventBasis(prep["ctx"], op, run["ncv"])
            basis.set_row_permutation(prep["perm"])
            if self._block_forcings:
                basis.set_block_forcings(True)
            if any(spec is not None for spec in self._sides):
                basis.set_weights(*self._weights_on_device(prep, self._sides, "resolvent_weights"))
            v0 = eps.start_vector(basis.n) if warm is None else np.asarray(warm, dtype=np.complex128)[prep["perm"]]
            out = basis.solve(nev, cfg.atol, cfg.max_it, v0=v0, seed=self._seed, max_out=nev, forcings=forcings)
            st = op.stats()
            basis_bytes = basis.basis_bytes
        finally:
            del basis  # (the basis goes before its operator)
            run.clear()
        if out["nconv"] < nev:
            logger.warning("Resolvent: %d of %d gains converged in %d restarts (next estimate %.3e)", out["nconv"], nev, out["restarts"],
                           out["next_unconverged"])
        return out, self._stats_of(out, st, basis_bytes, prepared_anew, time.time() - started)

    def solve(self, omega: float, forcings: bool = True, discount: float | None = None) -> ResolventResult:
        """Gains, responses and (``forcings=True``) forcings at the real frequency ``omega``: factorises ``A - (beta + i omega) M``
        with ``beta = discount`` (``None``: the solver's; a real shift, ``omega = 0`` at any ``beta``, runs on real factors) and
        iterates.  The responses are orthonormal in the response weight, ``q_j^H Qq q_k = delta_jk``, the forcings in the forcing
        weight, ``f_j^H Qf f_k = delta_jk``, with ``R Qf f_j = sigma_j q_j`` and ``R = ((beta + i omega) M - A)^-1``; both weights are
        ``M`` where the solver was given none.  A second call on the same solver keeps the context, the ordering, the LU analysis
        and the weights on the device."""
        omega = _real_frequency(omega)
        beta = self._discount if discount is None else _real_discount(discount)
        nev = self._cfg.num_modes
        out, stats = self._iterate(complex(beta, omega), nev, forcings)
        k = len(out["gains"])
        return ResolventResult(omega, out["gains"], out["responses"][:, :k], out["forcings"], out["estimates"], stats, beta)

    @staticmethod
    def _stats_of(out: dict, st: dict, basis_bytes: int, prepared_anew: bool, seconds_total: float) -> dict:
        return {"applies": out["applies"], "restarts": out["restarts"], "nconv": out["nconv"], "adjoint_solves": out["adjoint_solves"],
                "forward_solves": out["forward_solves"], "refinements": out["refined_adjoint"] + out["refined_forward"],
                "refined_adjoint": out["refined_adjoint"], "refined_forward": out["refined_forward"],
                "analysis_reused": bool(st.get("analysis_reused")), "max_rel_res": st.get("max_rel_res"), "basis_bytes": basis_bytes,
                "spmv_calls": st.get("spmv_calls"), "prepared_anew": prepared_anew,
                "seconds_factor": st.get("seconds_factor"), "seconds_solve": st.get("seconds_solve"), "seconds_expand": out["seconds_expand"],
                "seconds_dense": out["seconds_dense"], "seconds_restart": out["seconds_restart"], "seconds_total": seconds_total}

    def _lockstep_bytes_per_member(self, prep: dict) -> int:
        """Device bytes one member of a lockstep group keeps alive: its factor set by the memory plan of the prepared analysis
        (``lsa_ndlu_prepared_memory``), the two ``n x (ncv + 1)`` complex bases (three with the row permutation's output), the ten
        complex work vectors of the basis and its operator, and the values of ``C = A - shift M``."""
        n, ncv = prep["n"], min(self._cfg.ncv, prep["n"])
        return int(prep["ctx"].prepared_lu_bytes() + 3 * 16 * n * (ncv + 1) + 10 * 16 * n + 16 * prep["dA"].nnz)

    @staticmethod
    def _checked_max_batch(max_batch) -> int:
        if not isinstance(max_batch, (int, np.integer)) or isinstance(max_batch, bool) or max_batch < 1:
            raise ValueError(f"max_batch must be a positive integer, got {max_batch!r}")
        return int(max_batch)

    def plan_lockstep(self, shifts, max_batch: int = 8, *, bytes_per_member: int = 0, memory_budget: int = 0):
        """``(chunks, alone)``: the positions of ``shifts`` off the real axis in the order given, in chunks of at most
        ``min(max_batch, 16)`` members, cut further to ``memory_budget // bytes_per_member`` where both are given
        (:func:`Solver.batch.plan_batches`); and the positions of the real shifts, which run on real factors through :meth:`solve`."""
        from .batch import MAX_BATCH, batch_key, plan_batches

        self._checked_max_batch(max_batch)
        shifts = [complex(z) for z in shifts]
        cx = [i for i, z in enumerate(shifts) if z.imag != 0.0]
        alone = [i for i, z in enumerate(shifts) if z.imag == 0.0]
        if not cx:
            return [], alone
        # one solver, one pattern, one key: hashed once, not per frequency.  The key reads from the target whether the factors are
        # complex, so it is taken at the first complex shift and the solver's own target is put back: planning moves no state.
        kept = self._eps._target
        try:
            self._eps._target = shifts[cx[0]]
            key = batch_key(self._eps)
        finally:
            self._eps._target = kept
        plan = plan_batches([self._eps] * len(cx), min(int(max_batch), MAX_BATCH), bytes_per_problem=bytes_per_member, memory_budget=memory_budget,
                            keys=[key] * len(cx))
        if plan.alone:
            raise NotImplementedError(f"{self.NAME}: lockstep needs the exact LU on one GPU ({next(iter(plan.alone.values()))})")
        return [[cx[q] for q in g] for g in plan.groups], alone

    def _iterate_group(self, shifts, nev: int, forcings: bool):
        """The iterations at the complex ``shifts`` of one chunk in ONE library call (``lsa_resolvent_solve_batch``): every member's
        operator is opened on the one context, ordering and analysis (members after the first redo the pattern-only phase, as
        ``Solver.eigen.solve_batch(lockstep=True)`` does), the members advance in lockstep and each returns the bytes of its own
        :meth:`_iterate`.  Returns ``[(out, stats)]`` in order and leaves the call's counters in ``self.last_lockstep_info``."""
        import lsa_hip

        eps, cfg = self._eps, self._cfg
        started = time.time()
        runs, bases, anew = [], [], []
        try:
            for q, shift in enumerate(shifts):
                before = eps.prepared
                if q > 0:
                    # the prepared analysis went into the previous member's factorisation, which is alive: the pattern-only phase again
                    # (own_context: this solver's context is its own, not a batch group's shared one)
                    eps.redo_pattern_phase(own_context=True)
                run, prep = self._open_operator(shift)
                runs.append(run)
                anew.append(prep is not before)
                basis = lsa_hip.ResolventBasis(prep["ctx"], run["op"], run["ncv"])
                bases.append(basis)
                basis.set_row_permutation(prep["perm"])
                if self._block_forcings:
                    basis.set_block_forcings(True)
                if any(spec is not None for spec in self._sides):
                    basis.set_weights(*self._weights_on_device(prep, self._sides, "resolvent_weights"))
            v0 = eps.start_vector(bases[0].n)
            outs, info = lsa_hip.ResolventBasis.solve_batch(bases, nev, cfg.atol, cfg.max_it, v0s=v0, seed=self._seed, max_out=nev, forcings=forcings,
                                                            raise_on_error=False)
            sts = [run["op"].stats() for run in runs]
            basis_bytes = [b.basis_bytes for b in bases]
        finally:
            del bases[:]  # (the bases go before their operators)
            for run in runs:
                run.clear()
        self.last_lockstep_info.append(info)
        for out in outs:
            if isinstance(out, BaseException):
                raise out
        share = (time.time() - started) / len(shifts)
        results = []
        for z, out in enumerate(outs):
            if out["nconv"] < nev:
                logger.warning("Resolvent: %d of %d gains converged in %d restarts (next estimate %.3e)", out["nconv"], nev, out["restarts"],
                               out["next_unconverged"])
            stats = self._stats_of(out, sts[z], basis_bytes[z], anew[z], share)
            stats.update(lockstep=info["lockstep_steps"][z] > 0, lockstep_steps=info["lockstep_steps"][z], solo_steps=info["solo_steps"][z],
                         batch_size=len(shifts))
            results.append((out, stats))
        return results

    def _iterate_lockstep(self, shifts, nev: int, forcings: bool, max_batch: int, alone):
        """``[(out, stats)]`` for every shift, in order: the complex ones in lockstep chunks (cut against 0.8 of the free device
        memory), chunks of one and the real ones through ``alone(shift)``, the solo path."""
        self.last_lockstep_info = []
        self._checked_max_batch(max_batch)  # (refused before any device work)
        shifts = [complex(z) for z in shifts]
        first = next((z for z in shifts if z.imag != 0.0), None)
        if first is None:
            chunks, real = self.plan_lockstep(shifts, max_batch)
        else:
            prep, ctx, _ = self._prepare(first)
            free, _total = ctx.mem_info()
            chunks, real = self.plan_lockstep(shifts, max_batch, bytes_per_member=self._lockstep_bytes_per_member(prep), memory_budget=int(0.8 * free))
        results: list = [None] * len(shifts)
        for chunk in chunks:
            if len(chunk) == 1:
                results[chunk[0]] = alone(shifts[chunk[0]])
                continue
            for i, r in zip(chunk, self._iterate_group([shifts[i] for i in chunk], nev, forcings)):
                results[i] = r
        for i in real:
            results[i] = alone(shifts[i])
        return results

    def sweep(self, omegas, forcings: bool = True, lockstep: bool = False, max_batch: int = 8) -> list[ResolventResult]:
        """One result per frequency on ONE context, ordering and LU analysis: every frequency after the first refactorises only
        (``stats["analysis_reused"]``), and returns the bytes a fresh solver gives for it.  (Going between a real shift -- ``omega = 0``
        -- and a complex one changes the factors' scalar type and prepares anew.)

        ``lockstep=True``: the frequencies with a complex shift run in groups of up to ``min(max_batch, 16)`` -- fewer where the
        device memory does not hold that many factor sets -- whose members advance together, one batched launch per launch of a
        solo step and one read-back per round (``lsa_resolvent_solve_batch``).  Every frequency returns the bytes of the default;
        its stats gain ``lockstep``, ``lockstep_steps`` and ``solo_steps``.  Real shifts and groups of one go through :meth:`solve`;
        the results come back in the order of ``omegas``.  The counters of each group's call are left in ``self.last_lockstep_info``."""
        omegas = [_real_frequency(w) for w in omegas]
        if not lockstep:
            return [self.solve(w, forcings=forcings) for w in omegas]
        beta, nev = self._discount, self._cfg.num_modes

        def alone(shift):
            out, stats = self._iterate(shift, nev, forcings)
            stats.update(lockstep=False, lockstep_steps=0, solo_steps=out["applies"])
            return out, stats

        pairs = self._iterate_lockstep([complex(beta, w) for w in omegas], nev, forcings, max_batch, alone)
        return [ResolventResult(w, out["gains"], out["responses"][:, :len(out["gains"])], out["forcings"], out["estimates"], stats, beta)
                for w, (out, stats) in zip(omegas, pairs)]

    @staticmethod
    def map_order(points) -> list[int]:
        """The order in which :meth:`norm_map` visits its points: those off the real axis in the order given, then the real ones
        (real factors: one group, so the analysis is prepared at most twice)."""
        z = np.asarray(points, dtype=np.complex128).ravel()
        return [i for i in range(z.size) if z[i].imag != 0.0] + [i for i in range(z.size) if z[i].imag == 0.0]

    def _gain_at(self, z: complex, warm):
        """(sigma_1, response, stats) at one point of :meth:`norm_map`."""
        out, stats = self._iterate(complex(z), 1, False, warm)
        if len(out["gains"]) < 1:
            raise RuntimeError(f"norm_map: sigma_1 at z = {z!r} did not converge in {out['restarts']} restarts")
        return float(out["gains"][0]), out["responses"][:, 0], stats

    def norm_map(self, points, warm_start: bool = True, lockstep: bool = False, max_batch: int = 8) -> np.ndarray:
        """``sigma_1(z_k)`` of the (possibly weighted) resolvent ``(z_k M - A)^-1`` at complex points ``z_k``, in the shape of
        ``points``: ``1 / sigma_1`` is the epsilon-level of the energy-norm pseudospectrum.  One mode, no forcings, one context,
        ordering and analysis; the real points are visited as one group (:meth:`map_order`).  ``warm_start``: the start vector of a
        point is the previous point's response.  The statistics of every point, in the order given, are left in
        ``self.last_map_stats``.

        ``lockstep=True``: the points off the real axis run in lockstep groups of up to ``min(max_batch, 16)`` (see :meth:`sweep`).
        The members of a group start together, so warm starts cannot be chained: ``lockstep=True`` needs ``warm_start=False``, and
        returns the bytes of ``norm_map(points, warm_start=False)``."""
        if lockstep and warm_start:
            raise ValueError("norm_map: a lockstep group starts its points together and cannot chain warm starts: lockstep=True needs warm_start=False")
        z = np.asarray(points, dtype=np.complex128)
        flat = z.ravel()
        if not np.isfinite(flat).all():
            raise ValueError("norm_map: the points must be finite complex numbers")
        gains = np.zeros(flat.size)
        stats: list = [None] * flat.size
        if lockstep:
            def alone(shift):
                out, st = self._iterate(shift, 1, False)
                st.update(lockstep=False, lockstep_steps=0, solo_steps=out["applies"])
                return out, st

            for i, (out, st) in enumerate(self._iterate_lockstep([complex(p) for p in flat], 1, False, max_batch, alone)):
                if len(out["gains"]) < 1:
                    raise RuntimeError(f"norm_map: sigma_1 at z = {complex(flat[i])!r} did not converge in {out['restarts']} restarts")
                gains[i], stats[i] = float(out["gains"][0]), st
            self.last_map_stats = stats
            return gains.reshape(z.shape)
        warm = None
        for i in self.map_order(flat):
            gains[i], response, stats[i] = self._gain_at(complex(flat[i]), warm if warm_start else None)
            warm = response
        self.last_map_stats = stats
        return gains.reshape(z.shape)
