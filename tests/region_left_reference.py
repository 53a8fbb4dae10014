"""numpy / SuperLU restatement of the LEFT phase of the region eigensolver (``lsa_contour_solve_left``, ``Solver/region.py`` with
``two_sided=True``) and of the biorthonormalisation, on the S2k pencil of ``region_reference.py``.  Never imported by the product.

Sign and conjugation of the left quadrature, derived here and not taken from the product.  A left eigenvector ``w`` of ``(A, M)``
with ``w^H A = lam w^H M`` is a right eigenvector of the adjoint pencil: ``A^H w = mu M^H w``, ``mu = conj(lam)``.  The eigenvalues
``mu`` wanted lie inside the conjugate ellipse (centre ``conj(c)``, the same semi-axes).  Its spectral projector is
``P' = (1 / 2 pi i) oint (z' M^H - A^H)^-1 M^H dz'`` counter-clockwise; the midpoint rule of ``region_reference.nodes_and_weights``
on that ellipse has nodes ``z'_j = conj(c) + rx cos t_j + i ry sin t_j`` and weights ``w'_j = (ry cos t_j + i rx sin t_j) / N``.
Because ``t_j = 2 pi (j + 1/2) / N`` is symmetric about zero, ``{z'_j} = {conj(z_k)}``: node ``conj(z_k)`` sits at the angle ``-t_k``,
where the weight is ``(ry cos t_k - i rx sin t_k) / N = conj(w_k)``.  And ``conj(z_k) M^H - A^H = -(A - z_k M)^H = -C_k^H``.  Hence
``Q = sum_k conj(w_k) (-C_k^H)^-1 M^H Y = -sum_k conj(w_k) C_k^-H M^H Y``: the factorisations of ``C_k`` serve, solved in their
conjugate-transposed form (``splu(...).solve(b, trans="H")``).  ``test_region_left_cpu.py`` pins this against the quadrature built
directly on the adjoint pencil's own nodes and factorisations.

Biorthonormalisation: with the right vectors ``X`` and the left vectors ``W`` of the same ``count`` eigenvalues, ``G = W^H M X`` is
nonsingular (block diagonal over distinct eigenvalues up to the residuals), and ``W' = W G^-H`` has ``W'^H M X = I``: column ``i`` of
``W'`` is the left eigenvector of ``eigenvalues[i]``, with no pairing by value and whatever the clusters.  ``kappa_i = ||w'_i||
||M x_i|| / |w'_i^H M x_i|``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import region_reference as rr

# The relative deviation of kappa between this restatement and inverse iteration, as tests/test_region_left_cpu.py measures it (2.3e-10
# on R1, 9.2e-10 on R2), and what a comparison across summation orders (the GPU against this restatement) is allowed: ten times that.
KAPPA_DEVIATION = 1e-9
KAPPA_RTOL = 10.0 * KAPPA_DEVIATION


@dataclass
class LeftResult:
    eigenvalues: np.ndarray   # lam = conj(mu), the values in the caller's region
    eigenvectors: np.ndarray  # W: w^H A = lam w^H M, unit 2-norm
    residuals: np.ndarray     # ||A^H w - mu M^H w|| / (||A^H w|| + |mu| ||M^H w||)
    count: int
    complete: bool
    iterations: int


def left_quadrature(lus, w, MH, Y):
    """``Q = -sum_k conj(w_k) C_k^-H M^H Y`` on the factorisations ``lus`` of ``C_k = A - z_k M``."""
    B = MH @ Y
    return sum(-np.conj(wk) * lu.solve(B, trans="H") for wk, lu in zip(w, lus))


def left_solve(A, M, centre: complex, rx: float, ry: float, nodes: int, Y0: np.ndarray, atol: float = rr.ATOL, max_it: int = rr.MAX_IT) -> LeftResult:
    A, M = sp.csr_matrix(A), sp.csr_matrix(M)
    AH, MH = sp.csr_matrix(A.conj().T), sp.csr_matrix(M.conj().T)
    z, w = rr.nodes_and_weights(centre, rx, ry, nodes)
    lus = [spla.splu((A - zk * M).tocsc()) for zk in z]
    Y = np.asarray(Y0, dtype=np.complex128)
    stopped = False
    for it in range(1, max_it + 1):
        Q = left_quadrature(lus, w, MH, Y)
        U = rr.gram_orth(rr.gram_orth(Q))
        AU, MU = AH @ U, MH @ U
        mu, S = sla.eig(np.linalg.solve(U.conj().T @ MU, U.conj().T @ AU))
        RA, RM = AU @ S, MU @ S
        res = np.linalg.norm(RA - RM * mu, axis=0) / (np.linalg.norm(RA, axis=0) + np.abs(mu) * np.linalg.norm(RM, axis=0) + 1e-16)
        sel = rr.inside(np.conj(mu), centre, rx, ry)
        if np.all(res[sel] <= atol) and (sel.any() or it > 1):
            stopped = True
            break
        Y = U
    W = U @ S[:, sel]
    W = W / np.linalg.norm(W, axis=0)
    return LeftResult(np.conj(mu[sel]), W, res[sel], int(sel.sum()), bool(stopped and sel.sum() < U.shape[1]), it)


def biorthonormalise(M, X: np.ndarray, W: np.ndarray):
    """``(W G^-H, G, kappa)`` with ``G = W^H M X``."""
    MX = sp.csr_matrix(M) @ X
    G = W.conj().T @ MX
    Wb = W @ np.linalg.inv(G).conj().T
    kappa = np.linalg.norm(Wb, axis=0) * np.linalg.norm(MX, axis=0) / np.abs(np.sum(Wb.conj() * MX, axis=0))
    return Wb, G, kappa


def left_residuals(A, M, lam: np.ndarray, W: np.ndarray) -> np.ndarray:
    AW, MW = sp.csr_matrix(A).conj().T @ W, sp.csr_matrix(M).conj().T @ W
    return np.linalg.norm(AW - MW * np.conj(lam), axis=0) / (np.linalg.norm(AW, axis=0) + np.abs(lam) * np.linalg.norm(MW, axis=0) + 1e-16)


def kappa_by_inverse_iteration(A, M, lam: complex, x: np.ndarray, steps: int = 3, delta: float = 1e-7) -> float:
    """The independent reference: the left eigenvector of ``lam`` by ``steps`` of inverse iteration with
    ``splu((A - (lam + delta) M)^H)`` (each step amplifies the wanted direction by ``gap / delta``), then the definition of kappa."""
    A, M = sp.csr_matrix(A), sp.csr_matrix(M)
    lu = spla.splu(sp.csc_matrix((A - (lam + delta) * M).conj().T))
    MH = sp.csr_matrix(M.conj().T)
    w = np.random.default_rng(7).standard_normal(A.shape[0]) + 0j
    for _ in range(steps):
        w = lu.solve(MH @ w)
        w /= np.linalg.norm(w)
    Mx = M @ x
    return float(np.linalg.norm(w) * np.linalg.norm(Mx) / abs(np.vdot(w, Mx)))
