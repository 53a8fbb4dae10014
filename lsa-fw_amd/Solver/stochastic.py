"""Response to stochastic forcing on the MI355X path: the variance ``M q' = A q + f`` sustains under forcing that is white in time,
the structures that carry it (empirical orthogonal functions, EOFs) and the forcing structures that feed it (stochastic optimals).

With ``R(z) = (z M - A)^-1`` the response covariance of a stable pair is ``P = (1 / 2 pi) int R Qf R^H d omega``; the EOFs are the
eigenvectors of ``P Qq = (1 / 2 pi) int W(i omega) d omega``, ``W(z) = C^-1 Qf C^-H Qq`` with ``C = A - z M``: the operator a resolvent
step applies.  For real ``A``, ``M`` the integral over the whole axis is ``S = (1 / pi) sum_k w_k Re W(i omega_k)`` over quadrature
nodes ``omega_k >= 0``: a real operator, self-adjoint in the ``Qq``-semi-inner product.  The library runs a real thick-restart Lanczos
iteration on it with ``nodes`` factorisations of ``A - i omega_k M`` kept alive on one ordering and one LU analysis
(``lsa_stochastic_*``, ``csrc/stochastic.hip``)::

    cfg = StochasticConfig(num_modes=4, ncv=24, atol=1e-8, nodes=16)
    sf = StochasticForcingSolver(A, M, cfg)
    res = sf.solve(band=(0.0, 1.5))                    # Gauss-Legendre on [0, 1.5]: res.variances, res.modes, res.spectrum
    res = sf.solve(band=(0.0, np.inf), scale=0.5)      # the whole axis through omega = scale * tan(theta)
    res = sf.solve(omegas=w, weights=dw, kind="optimals")

**The results are those of the quadrature operator** ``S`` **the call defines, not of the integral**: whether ``nodes`` nodes resolve
the integrand is the caller's to check, by solving again with more.  Near sharp resonances the leading variances converge slowly in
``nodes`` (their sum converges much sooner); ``discount=beta`` evaluates ``W`` at ``beta + i omega`` and smooths the integrand, as it
does for the resolvent.  Forcing and response windows and weights mean what they mean in :class:`Solver.resolvent.ResolventSolver`
and are built on the device the same way (``CsrMatrix.windowed``).  ``batch_adjoint=True`` sends the adjoint solves of a step through
the batched transposed sweeps (same bits; off by default).

``solve(..., trace=32)`` (or a :class:`TraceConfig`) adds the total variance ``tr S`` -- the sum of ALL variances -- estimated by block
probes on the same handle and factor sets (``lsa_stochastic_trace``), deflated with the converged modes, and with it the share of the
total the leading modes carry (``res.total_variance``, ``res.captured``); ``total_variance(...)`` gives the trace alone, without an
eigen-iteration.  The trace is far more stable in ``nodes`` than the leading variances are.  Hutch++-style sketching, adaptive stopping
on a requested standard error, several ranks, complex pencils and refactorising factor sets when ``nodes`` of them do not fit are not
built.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field

import numpy as np

from .exact_lu import ExactLuFrontEnd, checked_side
from .resolvent import _real_discount
from .utils import PreconditionerType

logger = logging.getLogger(__name__)

KINDS = {"eofs": 0, "optimals": 1}
MEMORY_FRACTION = 0.8  # of the free device memory: what the kept factor sets may take (``solve_batch``'s rule)


@dataclass(frozen=True)
class StochasticConfig:
    num_modes: int = 4  # variances (with their modes) to compute
    ncv: int = 24  # Krylov subspace dimension
    atol: float = 1e-8  # relative tolerance on a variance: |beta y_mi| / theta_i
    max_it: int = 500  # restarts allowed
    nodes: int = 16  # quadrature nodes = factorisations kept alive (``band=`` rules; explicit ``omegas`` bring their own count)


@dataclass(frozen=True)
class TraceConfig:
    """The block-probe estimate of the total variance ``tr S`` behind ``solve(trace=...)``."""

    probes: "int | np.ndarray" = 32  # Rademacher probes generated on the device from ``seed``, or an ``n x R`` real array of the caller's own
    seed: int = 0
    deflate: bool = True  # remove the converged modes from the probes: they then resolve only ``tr S - sum(theta)``
    batch: int = 0  # probes per block solve (0: chosen by the library from the free memory, 8 at most)


@dataclass
class StochasticResult:
    """``Q`` below is the weight of the kind: the response weight ``Qq`` for EOFs, the forcing weight ``Qf`` for stochastic optimals
    (``M`` where the solver was given none)."""

    variances: np.ndarray  # eigenvalues of the quadrature operator, descending
    modes: np.ndarray  # n x k real, e_j^T Q e_k = delta_jk, the entry of largest magnitude positive
    kind: str  # "eofs" or "optimals"
    omegas: np.ndarray  # the quadrature nodes
    weights: np.ndarray  # ... and weights
    spectrum: np.ndarray  # k x N: [j, k] = node k's contribution to variances[j]; rows sum to variances
    estimates: np.ndarray  # relative residual estimates of the variances
    stats: dict = field(default_factory=dict)
    discount: float = 0.0
    # with ``solve(trace=...)`` (``None`` otherwise):
    total_variance: float | None = None  # the estimate of tr S, the sum of all variances of the quadrature operator
    total_variance_stderr: float | None = None  # its standard error over the probes (nan for one probe, 0 for the n unit vectors)
    captured: np.ndarray | None = None  # k cumulative fractions sum_{i <= j} variances[i] / total_variance
    captured_stderr: np.ndarray | None = None  # ... and their first-order errors
    node_totals: np.ndarray | None = None  # N: node k's share of total_variance, the frequency-resolved variance


def trace_summary(forms, variances=None, exact: bool = False) -> dict:
    """The estimate of ``tr S`` from the forms ``z_r^T S p_r`` of ``R`` probes deflated by modes with the given ``variances`` (``None``:
    no deflation): ``total = sum(variances) + mean(forms)`` and ``stderr = std(forms, ddof=1) / sqrt(R)`` (``nan`` for ``R = 1``).
    ``exact=True``: the probes were the ``n`` unit vectors, so ``total = sum(variances) + sum(forms)`` and ``stderr = 0``.  Returns a dict:
    ``total``, ``stderr``, ``remainder`` (the probes' part), ``exact``."""
    f = np.atleast_1d(np.asarray(forms, dtype=np.float64))
    if f.ndim != 1 or f.size < 1:
        raise ValueError(f"forms must be a non-empty vector, got shape {f.shape}")
    head = 0.0 if variances is None else float(np.sum(np.asarray(variances, dtype=np.float64)))
    if exact:
        rest, err = float(f.sum()), 0.0
    else:
        rest = float(f.mean())
        err = float(f.std(ddof=1) / math.sqrt(f.size)) if f.size > 1 else math.nan
    return {"total": head + rest, "stderr": err, "remainder": rest, "exact": bool(exact)}


def captured_fractions(variances, total: float, stderr: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """``(fractions, errors)``: the cumulative shares ``sum_{i <= j} variances[i] / total`` of the total variance and their first-order
    errors ``fraction * stderr / total`` (the variances themselves are taken as exact)."""
    if not (math.isfinite(total) and total > 0.0):
        raise ValueError(f"total = {total!r} must be positive and finite")
    frac = np.cumsum(np.asarray(variances, dtype=np.float64)) / float(total)
    return frac, frac * (float(stderr) / float(total))


def checked_trace(trace, n: int) -> "TraceConfig | None":
    """``solve``'s ``trace=`` as a :class:`TraceConfig` (``None`` stays ``None``; an int is a probe count).  ``ValueError`` for a count
    below 1, a probe array that is not ``n x R`` real with ``R >= 1``, or a negative batch.  Pure host logic."""
    if trace is None:
        return None
    if not isinstance(trace, TraceConfig):
        trace = TraceConfig(probes=trace)
    p = trace.probes
    if isinstance(p, (bool, np.bool_)):
        raise ValueError(f"trace: probes = {p!r} must be a count or an array")
    if isinstance(p, (int, np.integer)):
        if p < 1:
            raise ValueError(f"trace: probes = {int(p)} must be at least 1")
    else:
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[0] != n or p.shape[1] < 1 or not np.isrealobj(p):
            raise ValueError(f"trace: a probe array must be real with shape ({n}, R), R >= 1, got {p.shape} {p.dtype}")
        trace = TraceConfig(np.asfortranarray(p, dtype=np.float64), trace.seed, trace.deflate, trace.batch)
    if not isinstance(trace.batch, (int, np.integer)) or trace.batch < 0:
        raise ValueError(f"trace: batch = {trace.batch!r} must be 0 (chosen) or positive")
    return trace


def _unit_vectors(p) -> bool:
    return isinstance(p, np.ndarray) and p.shape[0] == p.shape[1] and np.array_equal(p, np.eye(p.shape[0]))


def gauss_legendre_band(a: float, b: float, nodes: int) -> tuple[np.ndarray, np.ndarray]:
    """Gauss-Legendre nodes and weights on ``[a, b]``, ``0 <= a < b < inf``."""
    if not (math.isfinite(a) and math.isfinite(b) and 0.0 <= a < b):
        raise ValueError(f"band = ({a!r}, {b!r}) must satisfy 0 <= a < b < inf (the whole axis: band=(0, inf) with scale=)")
    x, w = np.polynomial.legendre.leggauss(int(nodes))
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def tan_rule(scale: float, nodes: int) -> tuple[np.ndarray, np.ndarray]:
    """``[0, inf)`` through ``omega = scale * tan(theta)``: Gauss-Legendre in ``theta`` on ``[0, pi / 2]``, ``d omega = scale / cos^2(theta)
    d theta``."""
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale = {scale!r} must be a positive frequency")
    theta, w = gauss_legendre_band(0.0, 0.5 * math.pi, nodes)
    return scale * np.tan(theta), scale * w / np.cos(theta) ** 2


def quadrature(nodes: int, band=None, scale=None, omegas=None, weights=None) -> tuple[np.ndarray, np.ndarray]:
    """The nodes and weights a ``solve`` call names: ``band=(a, b)``, ``band=(0, inf)`` with ``scale``, or explicit arrays.
    ``ValueError`` for anything else, a negative frequency or a weight that is not positive."""
    if (band is None) == (omegas is None):
        raise ValueError("give either band=(a, b) or omegas= and weights=")
    if omegas is not None:
        if weights is None or band is not None or scale is not None:
            raise ValueError("explicit nodes come as omegas= and weights=, without band= or scale=")
        om, w = np.atleast_1d(np.asarray(omegas, dtype=np.float64)), np.atleast_1d(np.asarray(weights, dtype=np.float64))
        if om.ndim != 1 or om.shape != w.shape or om.size < 1:
            raise ValueError(f"omegas and weights must be one-dimensional and of one length, got {om.shape} and {w.shape}")
    else:
        if weights is not None:
            raise ValueError("weights= belongs to omegas=")
        a, b = (float(t) for t in band)
        if not isinstance(nodes, (int, np.integer)) or nodes < 1:
            raise ValueError(f"nodes = {nodes!r} must be at least 1")
        if math.isinf(b):
            if a != 0.0 or scale is None:
                raise ValueError("an unbounded band is band=(0, inf) with scale=")
            om, w = tan_rule(float(scale), nodes)
        else:
            if scale is not None:
                raise ValueError("scale= belongs to band=(0, inf)")
            om, w = gauss_legendre_band(a, b, nodes)
    if not np.isfinite(om).all() or (om < 0.0).any():
        raise ValueError("the frequencies must be finite and non-negative: the quadrature over omega >= 0 stands for the whole axis")
    if not np.isfinite(w).all() or (w <= 0.0).any():
        raise ValueError("the quadrature weights must be positive and finite")
    return om, w


def plan_factor_sets(nodes: int, bytes_per_set: int, free_bytes: int, fraction: float = MEMORY_FRACTION) -> int:
    """The bytes ``nodes`` kept factor sets need; ``MemoryError``, naming the bytes needed and the bytes available, when they exceed
    ``fraction`` of the free device memory.  Pure host arithmetic (the library applies the same rule before it factorises)."""
    need = int(nodes) * int(bytes_per_set)
    have = int(fraction * int(free_bytes))
    if need > have:
        fit = have // max(int(bytes_per_set), 1)
        raise MemoryError(f"stochastic forcing: {nodes} factor sets need {need} bytes, {fraction:g} of the {int(free_bytes)} bytes of free device "
                          f"memory hold {have}: at most {fit} nodes fit (refactorising sets node by node is not built)")
    return need


class StochasticForcingSolver(ExactLuFrontEnd):
    """EOFs and stochastic optimals of a real pair ``(A, M)`` on a frequency quadrature, with optional forcing and response windows
    or weights; thin shell around :class:`iEpsSolver` 's preparation (union pattern, nested-dissection ordering, permuted numbering,
    upload, pattern-only LU analysis) and ``lsa_hip.StochasticBasis``.  The results are those of the quadrature operator;
    convergence in ``nodes`` is the caller's to check, and ``discount`` smooths the integrand."""

    NAME = "Stochastic forcing"
    NEEDS_M = "the variance is measured in the M-inner product"
    NEEDS_LU = "every node of the quadrature is a pair of solves on its factors"
    REAL_A = "Stochastic forcing needs a real A: the quadrature over omega >= 0 stands for the whole axis only for a real pencil"
    REAL_M = "Stochastic forcing needs a real M (the M-inner product); M is complex"

    def __init__(self, A, M, cfg: StochasticConfig | None = None, *, device: int = 0, layout: str = "single",
                 pc_type: PreconditionerType = PreconditionerType.LU, ilu_levels: int | None = None, seed: int = 0,
                 ksp_rtol: float | None = None, forcing_window=None, response_window=None, forcing_weight=None, response_weight=None,
                 discount: float = 0.0, batch_forward: bool = True, batch_adjoint: bool = False) -> None:
        A, M, _, Ms = self._checked_pencil(A, M)
        self._sides = (checked_side("forcing", forcing_window, forcing_weight, Ms), checked_side("response", response_window, response_weight, Ms))
        self._discount = _real_discount(discount)
        self._cfg = cfg = cfg if cfg is not None else StochasticConfig()
        if cfg.num_modes < 1:
            raise ValueError("num_modes must be at least 1")
        if cfg.ncv <= cfg.num_modes:
            raise ValueError(f"ncv = {cfg.ncv} must exceed num_modes = {cfg.num_modes}")
        if not isinstance(cfg.nodes, (int, np.integer)) or cfg.nodes < 1:
            raise ValueError(f"nodes = {cfg.nodes!r} must be at least 1")
        self._set_up(A, M, cfg.atol, cfg.max_it, (cfg.num_modes, cfg.ncv), device=device, layout=layout, pc_type=pc_type, ilu_levels=ilu_levels,
                     seed=seed, ksp_rtol=ksp_rtol)
        # the forward solves of a step through the batched sweeps: same bits, and 0.79-0.92 of the default's time per step on every
        # case measured, so the front end switches it on; a new library handle has it off
        self._batch_forward = bool(batch_forward)
        # the adjoint solves through the batched transposed sweeps and their check products in groups of 16 per launch: same bits;
        # off until its measurement has been through the GPU suite
        self._batch_adjoint = bool(batch_adjoint)
        self._force_refinement = False  # (tests: every solve with the refinement step)

    @property
    def config(self) -> StochasticConfig:
        return self._cfg

    def solve(self, band=None, *, scale: float | None = None, omegas=None, weights=None, kind: str = "eofs", discount: float | None = None,
              trace: "int | TraceConfig | None" = None) -> StochasticResult:
        """The leading variances and modes of the quadrature operator over ``band=(a, b)`` (Gauss-Legendre, ``cfg.nodes`` nodes),
        ``band=(0, inf)`` with ``scale=s`` (``omega = s tan(theta)``) or explicit ``omegas`` and ``weights``.  ``kind="eofs"``: the
        response structures, orthonormal in ``Qq``; ``kind="optimals"``: the forcing structures, orthonormal in ``Qf``.  A second call
        on the same solver keeps the context, the ordering, the LU analysis and the weights on the device.  ``trace=`` (a probe count
        or a :class:`TraceConfig`): after the modes converge, the block-probe estimate of the total variance on the same handle and
        factor sets fills ``total_variance``, ``captured`` and ``node_totals`` of the result; everything else is what the call returns
        without it."""
        import lsa_hip

        if kind not in KINDS:
            raise ValueError(f"kind = {kind!r} must be 'eofs' or 'optimals'")
        trace = checked_trace(trace, self._n)
        om, w = quadrature(self._cfg.nodes, band, scale, omegas, weights)
        beta = self._discount if discount is None else _real_discount(discount)
        cfg, nev = self._cfg, self._cfg.num_modes
        shifts = beta + 1j * om
        started = time.time()
        prep, ctx, perm = self._prepare(complex(beta, max(float(om.max()), 1.0)))  # (never real: the analysis is prepared for complex factors)
        try:
            plan_factor_sets(om.size, ctx.prepared_lu_bytes(), ctx.mem_info()[0])
        except ValueError:  # (no analysis parked in the context: the library judges on the first set's)
            pass
        basis = None
        try:
            basis = lsa_hip.StochasticBasis(ctx, prep["dA"], prep["dM"], shifts, w, min(cfg.ncv, self._n), ksp_rtol=self._ksp_rtol)
            basis.set_row_permutation(perm)
            if any(spec is not None for spec in self._sides):
                basis.set_weights(*self._weights_on_device(prep, self._sides, "stochastic_weights"))
            basis.set_kind(KINDS[kind])
            if self._batch_forward:
                basis.set_batch_forward(True)
            if self._batch_adjoint:
                basis.set_batch_adjoint(True)
            if self._force_refinement:
                basis.set_refinement(True)
            rng = np.random.default_rng(self._seed)
            out = basis.solve(nev, cfg.atol, cfg.max_it, v0=rng.standard_normal(self._n)[perm], seed=self._seed, max_out=nev)
            batches = basis.info()  # (the grouped sweep calls of the iteration alone, like its solve counts: before the spectrum's applies)
            k = len(out["variances"])
            spectrum = np.zeros((k, om.size))
            for j in range(k):  # one apply per mode: node k's share of e_j^T Q S e_j
                spectrum[j] = basis.apply(np.ascontiguousarray(out["modes"][perm, j]))[1]
            info = basis.info()
            traced = None
            if trace is not None:  # (after everything else: what a solve without trace= returns is in hand)
                kc = min(int(out["nconv"]), k) if trace.deflate else 0
                traced = self._trace(basis, trace, out["modes"][:, :kc] if kc else None)
        finally:
            del basis  # (the handle goes before the matrices it borrows)
        if out["nconv"] < nev:
            logger.warning("Stochastic forcing: %d of %d variances converged in %d restarts (next estimate %.3e)", out["nconv"], nev, out["restarts"],
                           out["next_unconverged"])
        st = info["solver"]
        stats = {"applies": out["applies"], "restarts": out["restarts"], "nconv": out["nconv"], "nodes": int(om.size),
                 "adjoint_solves": out["adjoint_solves"], "forward_solves": out["forward_solves"],
                 "refined_adjoint": out["refined_adjoint"], "refined_forward": out["refined_forward"],
                 "refinements": out["refined_adjoint"] + out["refined_forward"], "backward_accepted": st["backward_accepted"],
                 "max_rel_res": st["max_rel_res"], "analysis_reused": bool(st["analysis_reused"]), "batch_forward": self._batch_forward,
                 "batch_adjoint": bool(info["batch_adjoint"]), "adjoint_batches": batches["adjoint_batches"], "forward_batches": batches["forward_batches"],
                 "stochastic_bytes": info["bytes"], "seconds_factor": info["seconds_factor"], "seconds_solve": info["seconds_solve"],
                 "seconds_product": info["seconds_product"], "seconds_solve_adjoint": info["seconds_solve_adjoint"],
                 "seconds_product_adjoint": info["seconds_product_adjoint"], "seconds_dense": info["seconds_dense"], "seconds_expand": out["seconds_expand"],
                 "seconds_restart": out["seconds_restart"], "seconds_total": time.time() - started}
        res = StochasticResult(out["variances"], out["modes"], kind, om, w, spectrum, out["estimates"], stats, beta)
        if traced is not None:
            kc = min(int(out["nconv"]), k) if trace.deflate else 0
            summary = trace_summary(traced["forms"], out["variances"][:kc] if kc else None, exact=traced["exact"])
            res.total_variance, res.total_variance_stderr = summary["total"], summary["stderr"]
            res.captured, res.captured_stderr = captured_fractions(out["variances"], summary["total"], summary["stderr"])
            res.node_totals = spectrum[:kc].sum(axis=0) + traced["node_rest"]
            stats["trace"] = traced["stats"]
        return res

    @staticmethod
    def _trace(basis, trace: TraceConfig, modes) -> dict:
        """The library's estimator on ``basis``: the forms, node ``k``'s share of the probes' part of the total, the library's stats."""
        p = trace.probes
        given = isinstance(p, np.ndarray)
        out = basis.trace(p.shape[1] if given else int(p), seed=trace.seed, probes=p if given else None, modes=modes, batch=int(trace.batch))
        exact = given and _unit_vectors(p)
        rest = out["node_terms"].sum(axis=1) if exact else out["node_terms"].mean(axis=1)
        return {"forms": out["forms"], "node_rest": rest, "stats": out["stats"], "exact": exact}

    def total_variance(self, band=None, *, scale: float | None = None, omegas=None, weights=None, probes=32, seed: int = 0, discount: float | None = None,
                       kind: str = "eofs", batch: int = 0) -> tuple[float, float, np.ndarray]:
        """``(total, stderr, node_totals)``: the block-probe estimate of ``tr S`` of the quadrature operator the arguments name (as
        :meth:`solve`'s), its standard error over the probes, and node ``k``'s share of it, without an eigen-iteration.  ``probes``: a
        count of Rademacher probes generated from ``seed``, or an ``n x R`` real array (the ``n`` unit vectors give the trace itself).  The
        library's stats of the call stay in ``self.trace_stats``."""
        import lsa_hip

        if kind not in KINDS:
            raise ValueError(f"kind = {kind!r} must be 'eofs' or 'optimals'")
        trace = checked_trace(TraceConfig(probes=probes, seed=seed, deflate=False, batch=batch), self._n)
        om, w = quadrature(self._cfg.nodes, band, scale, omegas, weights)
        beta = self._discount if discount is None else _real_discount(discount)
        prep, ctx, perm = self._prepare(complex(beta, max(float(om.max()), 1.0)))
        try:
            plan_factor_sets(om.size, ctx.prepared_lu_bytes(), ctx.mem_info()[0])
        except ValueError:
            pass
        basis = None
        try:
            basis = lsa_hip.StochasticBasis(ctx, prep["dA"], prep["dM"], beta + 1j * om, w, 1, ksp_rtol=self._ksp_rtol)
            basis.set_row_permutation(perm)
            if any(spec is not None for spec in self._sides):
                basis.set_weights(*self._weights_on_device(prep, self._sides, "stochastic_weights"))
            basis.set_kind(KINDS[kind])
            if self._force_refinement:
                basis.set_refinement(True)
            traced = self._trace(basis, trace, None)
        finally:
            del basis
        summary = trace_summary(traced["forms"], None, exact=traced["exact"])
        self.trace_stats = traced["stats"]
        return summary["total"], summary["stderr"], traced["node_rest"]
