"""Region eigensolver on the MI355X path: ALL eigenvalues of ``A x = lambda M x`` inside a contour, with a statement of completeness.

:class:`Solver.eigen.EigenSolver` answers "which eigenvalues lie nearest this target"; a Krylov-Schur run proves nothing about what
it did not find.  Stability analysis asks "is anything in this part of the right half plane?" of a non-symmetric pencil.  The library
answers with a contour-integral (FEAST-type) subspace iteration (``lsa_contour_*``, ``csrc/contour.hip``): the spectral projector of
the region is applied to a block of ``subspace`` vectors by a quadrature over ``nodes`` points of an ellipse, each a block solve on
a nested-dissection LU of ``A - z_k M``; the Ritz pairs of the projected pencil converge to the eigenpairs inside::

    cfg = RegionConfig(nodes=16, subspace=48, atol=1e-10, max_it=20)
    rs = RegionEigenSolver(A, M, cfg)
    res = rs.solve(Ellipse(0.018 + 0.738j, 0.12, 0.12))   # res.eigenvalues, res.count, res.complete
    res = rs.solve(Rectangle(-0.05, 0.1, 0.65, 0.8))      # the circumscribing ellipse, filtered to the rectangle

``complete`` is true when the iteration stopped because every Ritz value inside the ellipse had converged (an iteration that shows
none inside is confirmed by a second one first) AND directions of the subspace were left over: then the ``count`` eigenvalues returned are all there are.  ``subspace`` must exceed the count inside
generously (a dense spectrum next to the contour slows the iteration down to the quadrature's filter at the ``(subspace + 1)``-th
nearest eigenvalue); ``estimate`` (a stochastic estimate of the count, from the first quadrature) helps sizing it.

``RegionConfig(two_sided=True)`` adds the left phase: the same iteration on the adjoint pencil ``(A^H, M^H)``, whose node matrices on
the conjugate contour are ``(A - z_k M)^H`` -- the factor sets of the right phase, no second factorisation
(``lsa_contour_solve_left``).  From the same start block it returns ``left_eigenvalues`` / ``left_residuals_raw`` as the phase found
them and, when ``left_complete``, ``left_eigenvectors = W G^-H`` with ``G = W^H M X`` (so column ``i`` belongs to ``eigenvalues[i]``
and ``W^H M X = I``: no pairing by nearest value, clusters included), their residuals ``left_residuals`` against ``eigenvalues[i]``,
and the eigenvalue condition numbers ``kappa_i = ||w_i|| ||M x_i|| / |w_i^H M x_i|``.  ``left_complete`` needs the left phase
complete, its count equal to ``count``, and ``G`` numerically nonsingular: ``sigma_min(G) > count * eps * sigma_max(G)`` (the rank
rule of ``numpy.linalg.matrix_rank``); otherwise the three stay ``None`` and a warning names the condition.

The conjugate-node saving for real pencils, two-sided (oblique) projection inside the iteration, automatic growth of the subspace
and more than one GPU are not built.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field

import numpy as np

from .exact_lu import ExactLuFrontEnd
from .utils import PreconditionerType

logger = logging.getLogger(__name__)


def _finite(*values) -> bool:
    return all(isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) for v in values)


@dataclass(frozen=True)
class Ellipse:
    """``((Re z - Re centre) / rx)^2 + ((Im z - Im centre) / ry)^2 < 1``."""

    centre: complex
    rx: float
    ry: float

    def __post_init__(self):
        c = complex(self.centre)
        if not (_finite(c.real, c.imag, self.rx, self.ry) and self.rx > 0 and self.ry > 0):
            raise ValueError(f"Ellipse needs a finite centre and positive finite semi-axes, got centre={self.centre!r}, rx={self.rx!r}, ry={self.ry!r}")

    def ellipse(self) -> "Ellipse":
        return self

    def contains(self, z) -> np.ndarray:
        z, c = np.asarray(z, dtype=np.complex128), complex(self.centre)
        return ((z.real - c.real) / self.rx) ** 2 + ((z.imag - c.imag) / self.ry) ** 2 < 1.0


@dataclass(frozen=True)
class Rectangle:
    """``a < Re z < b`` and ``c < Im z < d`` (the arguments of ``set_interval_complex``).  The contour is the circumscribing ellipse,
    with semi-axes ``sqrt(2)`` times the half-widths; eigenpairs and ``count`` are filtered to the rectangle, ``complete`` refers to
    the ellipse and therefore covers the rectangle."""

    a: float
    b: float
    c: float
    d: float

    def __post_init__(self):
        if not (_finite(self.a, self.b, self.c, self.d) and self.a < self.b and self.c < self.d):
            raise ValueError(f"Rectangle needs finite a < b and c < d, got ({self.a!r}, {self.b!r}, {self.c!r}, {self.d!r})")

    def ellipse(self) -> Ellipse:
        return Ellipse(complex(0.5 * (self.a + self.b), 0.5 * (self.c + self.d)), math.sqrt(2.0) * 0.5 * (self.b - self.a),
                       math.sqrt(2.0) * 0.5 * (self.d - self.c))

    def contains(self, z) -> np.ndarray:
        z = np.asarray(z, dtype=np.complex128)
        return (z.real > self.a) & (z.real < self.b) & (z.imag > self.c) & (z.imag < self.d)


def contour_nodes(ellipse: Ellipse, nodes: int) -> tuple[np.ndarray, np.ndarray]:
    """Nodes ``z_k = c + rx cos t_k + i ry sin t_k`` and weights ``w_k = (ry cos t_k + i rx sin t_k) / N`` at ``t_k = 2 pi (k + 1/2) / N``
    (the half step keeps every node off the real axis): ``sum_k w_k / (z_k - lambda)`` is the midpoint rule for
    ``(1 / 2 pi i) oint dz / (z - lambda)``.  The library computes the same numbers in ``lsa_contour_create``."""
    t = 2.0 * np.pi * (np.arange(nodes) + 0.5) / nodes
    c = complex(ellipse.centre)
    return c + ellipse.rx * np.cos(t) + 1j * ellipse.ry * np.sin(t), (ellipse.ry * np.cos(t) + 1j * ellipse.rx * np.sin(t)) / nodes


@dataclass(frozen=True)
class RegionConfig:
    nodes: int = 16  # quadrature nodes on the ellipse (even, at least 4): one factorisation each
    subspace: int = 48  # columns of the block (2..128): must exceed the count inside generously
    atol: float = 1e-10  # residual ||A x - lam M x|| / (||A x|| + |lam| ||M x||) of every Ritz pair inside
    max_it: int = 20  # iterations allowed
    keep_factors: bool | None = None  # all factor sets alive / one refactorised per node and iteration / None: by the free memory
    batch_nodes: bool = False  # solve an iteration's block on all nodes in lockstep (kept factor sets, one more block per node); same bytes
    two_sided: bool = False  # after the right phase, the left phase on the same factor sets: left eigenvectors and condition numbers


@dataclass
class RegionResult:
    eigenvalues: np.ndarray  # inside the region, nearest the centre first
    eigenvectors: np.ndarray  # n x count complex, unit 2-norm, canonical phase, the caller's row order
    residuals: np.ndarray
    count: int
    complete: bool  # every Ritz value inside the ellipse converged and the subspace had directions to spare
    estimate: float  # stochastic estimate of the count inside the ellipse (first quadrature): for sizing `subspace`
    iterations: int
    stats: dict = field(default_factory=dict)
    # two_sided=True only (else None): the left phase as it returned, filtered by the region ...
    left_eigenvalues: np.ndarray | None = None
    left_residuals_raw: np.ndarray | None = None
    left_complete: bool | None = None  # the left phase completed, found `count` values, and G = W^H M X is numerically nonsingular
    # ... and, when left_complete: W G^-H (column i belongs to eigenvalues[i], W^H M X = I), its residuals against eigenvalues[i]
    # (||A^H w - conj(lam) M^H w|| / (||A^H w|| + |lam| ||M^H w||)), and kappa_i = ||w_i|| ||M x_i|| / |w_i^H M x_i|
    left_eigenvectors: np.ndarray | None = None
    left_residuals: np.ndarray | None = None
    condition_numbers: np.ndarray | None = None


def _check_config(cfg: RegionConfig) -> None:
    if not isinstance(cfg.nodes, (int, np.integer)) or cfg.nodes < 4 or cfg.nodes % 2:
        raise ValueError(f"nodes = {cfg.nodes!r} must be an even number of at least 4")
    if not isinstance(cfg.subspace, (int, np.integer)) or not 2 <= cfg.subspace <= 128:
        raise ValueError(f"subspace = {cfg.subspace!r} must lie between 2 and 128")
    if not (_finite(cfg.atol) and cfg.atol > 0):
        raise ValueError(f"atol = {cfg.atol!r} must be positive")
    if not isinstance(cfg.max_it, (int, np.integer)) or cfg.max_it < 1:
        raise ValueError(f"max_it = {cfg.max_it!r} must be at least 1")
    if cfg.keep_factors not in (None, True, False):
        raise ValueError(f"keep_factors = {cfg.keep_factors!r} must be True, False or None")
    if not isinstance(cfg.batch_nodes, (bool, np.bool_)):
        raise ValueError(f"batch_nodes = {cfg.batch_nodes!r} must be True or False")
    if not isinstance(cfg.two_sided, (bool, np.bool_)):
        raise ValueError(f"two_sided = {cfg.two_sided!r} must be True or False")
    if cfg.batch_nodes and cfg.keep_factors is False:
        raise ValueError("batch_nodes = True needs the factor sets of all nodes alive: keep_factors = False refactorises one set node by node")


class RegionEigenSolver(ExactLuFrontEnd):
    """All eigenvalues of ``(A, M)`` inside a region; thin shell around :class:`iEpsSolver` 's preparation (union pattern,
    nested-dissection ordering, permuted numbering, upload, pattern-only LU analysis) and ``lsa_hip.ContourSolver``."""

    NAME = "The region eigensolver"
    NEEDS_M = "the contour integral is that of the pencil (A, M)"
    NEEDS_LU = "every node of the contour is a block solve on its factors"
    REAL_M = "The region eigensolver needs a real M; M is complex"
    SYMMETRIC_M = False

    def __init__(self, A, M, cfg: RegionConfig | None = None, *, device: int = 0, layout: str = "single",
                 pc_type: PreconditionerType = PreconditionerType.LU, ilu_levels: int | None = None, seed: int = 0,
                 ksp_rtol: float | None = None) -> None:
        A, M, _, _ = self._checked_pencil(A, M)
        self._cfg = cfg if cfg is not None else RegionConfig()
        _check_config(self._cfg)
        if self._cfg.subspace > A.shape[0]:
            raise ValueError(f"subspace = {self._cfg.subspace} exceeds the problem size {A.shape[0]}")
        self._set_up(A, M, self._cfg.atol, self._cfg.max_it, None, device=device, layout=layout, pc_type=pc_type, ilu_levels=ilu_levels, seed=seed,
                     ksp_rtol=ksp_rtol)

    @property
    def config(self) -> RegionConfig:
        return self._cfg

    def start_block(self) -> np.ndarray:
        """The default start block: ``n x subspace`` complex normal from ``default_rng(seed)``, in the caller's row order."""
        rng = np.random.default_rng(self._seed)
        shape = (self._n, self._cfg.subspace)
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    def _keep_factors(self, ctx) -> bool:
        """``cfg.keep_factors``, or whether ``nodes`` factor sets and the blocks (six, and one more per node under ``batch_nodes``)
        fit 0.8 of the free device memory."""
        if self._cfg.keep_factors is not None:
            return bool(self._cfg.keep_factors)
        blocks = 6 + (self._cfg.nodes if self._cfg.batch_nodes else 0)
        try:
            need = self._cfg.nodes * ctx.prepared_lu_bytes() + blocks * 16 * self._n * self._cfg.subspace
        except ValueError:  # (no analysis parked in the context: nothing to size by)
            return False
        return need <= 0.8 * ctx.mem_info()[0]

    def solve(self, region, Y0: np.ndarray | None = None) -> RegionResult:
        """The eigenpairs inside ``region`` (:class:`Ellipse` or :class:`Rectangle`) from the start block ``Y0`` (``n x subspace``,
        the caller's row order; default :meth:`start_block`).  A second call keeps the context, the ordering and the LU analysis."""
        import lsa_hip

        if not isinstance(region, (Ellipse, Rectangle)):
            raise ValueError(f"region must be an Ellipse or a Rectangle, got {region!r}")
        ell, cfg = region.ellipse(), self._cfg
        if Y0 is None:
            Y0 = self.start_block()
        Y0 = np.asarray(Y0, dtype=np.complex128)
        if Y0.shape != (self._n, cfg.subspace):
            raise ValueError(f"Y0 must have shape ({self._n}, {cfg.subspace}), got {Y0.shape}")
        started = time.time()
        z, _ = contour_nodes(ell, cfg.nodes)
        prep, ctx, perm = self._prepare(complex(z[0]))  # (a node is never real: the analysis is prepared for complex factors)
        keep = self._keep_factors(ctx)
        batch = bool(cfg.batch_nodes) and keep
        if cfg.batch_nodes and not batch:
            logger.warning("Region: batch_nodes is set, but %d factor sets and %d solution blocks do not fit the free device memory: the factors "
                           "are not kept and the nodes are solved one by one", cfg.nodes, cfg.nodes)
        cs = None
        try:
            cs = lsa_hip.ContourSolver(ctx, prep["dA"], prep["dM"], cfg.nodes, ell.centre, ell.rx, ell.ry, cfg.subspace, keep_factors=keep,
                                       ksp_rtol=self._ksp_rtol, batch_nodes=batch)
            cs.set_row_permutation(perm)
            out = cs.solve(cfg.atol, cfg.max_it, np.asfortranarray(Y0[perm]))
            left = cs.solve_left(cfg.atol, cfg.max_it, np.asfortranarray(Y0[perm])) if cfg.two_sided else None
            info = cs.info()
            binfo = cs.batch_info()
            linfo = cs.left_info() if cfg.two_sided else None
        finally:
            del cs  # (the handle goes before the matrices it borrows)
        lam, X, res = out["eigenvalues"], out["eigenvectors"], out["residuals"]
        if not out["complete"]:
            if out["inside"] >= out["rank"]:
                logger.warning("Region: the subspace is full: all %d Ritz values lie inside the contour after %d iterations, so eigenvalues may be "
                               "missing; raise `subspace` (now %d; the estimate of the count inside is %.1f)", out["rank"], out["iterations"],
                               cfg.subspace, out["estimate"])
            else:
                logger.warning("Region: max_it = %d reached with %d of %d Ritz values inside the contour converged (subspace %d, estimate of the "
                               "count inside %.1f)", cfg.max_it, out["converged_inside"], out["inside"], cfg.subspace, out["estimate"])
        sel = region.contains(lam)
        st = info["solver"]
        stats = {"iterations": out["iterations"], "rank": out["rank"], "inside_ellipse": out["inside"], "converged_inside": out["converged_inside"],
                 "block_solves": out["block_solves"], "refined_solves": out["refined_solves"], "backward_accepted": out["backward_accepted"],
                 "max_rel_res": out["worst_rel_res"], "factors_kept": info["kept"], "nodes": info["nodes"],
                 "contour_bytes": info["bytes"], "analysis_reused": bool(st["analysis_reused"]), "seconds_factor": info["seconds_factor"],
                 "seconds_solve": info["seconds_solve"], "seconds_product": info["seconds_product"], "seconds_gram": info["seconds_gram"],
                 "seconds_dense": info["seconds_dense"], "seconds_total": time.time() - started, "batch_nodes": binfo["enabled"],
                 "batched_groups": binfo["groups"], "batched_columns": binfo["batched_columns"]}
        result = RegionResult(lam[sel], np.asfortranarray(X[:, sel]), res[sel], int(np.count_nonzero(sel)), bool(out["complete"]),
                              float(out["estimate"]), int(out["iterations"]), stats)
        if left is not None:
            stats["left"] = {"iterations": left["iterations"], "rank": left["rank"], "inside_ellipse": left["inside"],
                             "converged_inside": left["converged_inside"], "block_solves": left["block_solves"],
                             "refined_solves": left["refined_solves"], "backward_accepted": left["backward_accepted"],
                             "max_rel_res": left["worst_rel_res"], "seconds_factor": linfo["seconds_factor"], "seconds_solve": linfo["seconds_solve"],
                             "seconds_product": linfo["seconds_product"], "seconds_gram": linfo["seconds_gram"], "seconds_dense": linfo["seconds_dense"],
                             "batched_groups": linfo["groups"], "batched_columns": linfo["batched_columns"], "serial_columns": linfo["serial_columns"]}
            self._biorthonormalise(result, region, left, prep)
            stats["seconds_total"] = time.time() - started
        return result

    def _biorthonormalise(self, result: RegionResult, region, left: dict, prep: dict) -> None:
        """The left fields of ``result`` from the left phase's pairs: ``G = W^H M X`` (``lsa_spmm``, ``lsa_block_gram``), ``W G^-H``, the
        residuals of its columns against ``eigenvalues[i]`` (``lsa_spmm_transpose``) and ``kappa_i``."""
        import lsa_hip

        lsel = region.contains(left["eigenvalues"])
        result.left_eigenvalues, result.left_residuals_raw = left["eigenvalues"][lsel], left["residuals"][lsel]
        W, c, n = left["eigenvectors"][:, lsel], result.count, self._n
        why = None
        if not left["complete"]:
            why = (f"the left phase did not complete ({left['converged_inside']} of {left['inside']} Ritz values inside converged in "
                   f"{left['iterations']} iterations, rank {left['rank']})")
        elif W.shape[1] != c:
            why = f"the left phase found {W.shape[1]} eigenvalues in the region, the right phase {c}"
        elif c > 0:
            ctx, perm = prep["ctx"], prep["perm"]
            block = lambda V: lsa_hip.DeviceVector.from_numpy(ctx, np.asfortranarray(V[perm]).reshape(-1, order="F"))  # noqa: E731
            host = lambda d: d.numpy().reshape((n, c), order="F")  # noqa: E731
            dMX = lsa_hip.DeviceVector(ctx, n * c, np.complex128)
            prep["dM"].matmat(block(result.eigenvectors), dMX, c)
            G = lsa_hip.block_gram(ctx, n, block(W), c, dMX, c)
            sv = np.linalg.svd(G, compute_uv=False)
            if not (np.all(np.isfinite(sv)) and sv[-1] > c * np.finfo(float).eps * sv[0]):
                why = f"G = W^H M X is numerically singular (singular values from {sv[0]:.3e} down to {sv[-1]:.3e})"
            else:
                Wb = W @ np.linalg.inv(G).conj().T
                dW, dAW, dMW = block(Wb), lsa_hip.DeviceVector(ctx, n * c, np.complex128), lsa_hip.DeviceVector(ctx, n * c, np.complex128)
                prep["dA"].matmat_transpose(dW, dAW, c, conj=True)
                prep["dM"].matmat_transpose(dW, dMW, c, conj=True)
                AW, MW, MX, lam = host(dAW), host(dMW), host(dMX), result.eigenvalues
                result.left_eigenvectors = np.asfortranarray(Wb)
                result.left_residuals = np.linalg.norm(AW - MW * lam.conj(), axis=0) / (np.linalg.norm(AW, axis=0) + np.abs(lam) * np.linalg.norm(MW, axis=0) + 1e-16)
                wMx = np.sum(Wb[perm].conj() * MX, axis=0)
                result.condition_numbers = np.linalg.norm(Wb, axis=0) * np.linalg.norm(MX, axis=0) / np.abs(wMx)
        else:
            result.left_eigenvectors = np.zeros((n, 0), dtype=np.complex128, order="F")
            result.left_residuals, result.condition_numbers = np.zeros(0), np.zeros(0)
        result.left_complete = why is None
        if why is not None:
            logger.warning("Region: no left eigenvectors and condition numbers: %s", why)

    def sweep(self, regions, Y0: np.ndarray | None = None) -> list[RegionResult]:
        """One result per region on ONE context, ordering and LU analysis (``stats["analysis_reused"]``); every region returns the
        bytes a fresh solver gives for it."""
        regions = list(regions)
        for r in regions:
            if not isinstance(r, (Ellipse, Rectangle)):
                raise ValueError(f"region must be an Ellipse or a Rectangle, got {r!r}")
        return [self.solve(r, Y0) for r in regions]
