"""numpy / SuperLU restatement of the region eigensolver (``csrc/contour.hip``, ``Solver/region.py``), and the dense ground truth of
the S2k cylinder pencil its tests are pinned against.  Never imported by the product.

The algorithm, on an ellipse with centre ``c`` and semi-axes ``rx``, ``ry``: nodes ``z_k = c + rx cos t_k + i ry sin t_k`` at
``t_k = 2 pi (k + 1/2) / N``, weights ``w_k = (ry cos t_k + i rx sin t_k) / N``.  One iteration on the block ``Y``:
``Q = -sum_k w_k (A - z_k M)^-1 M Y``; ``U`` = ``Q`` orthonormalised twice through its Gram matrix (Hermitian eigen-decomposition,
directions below ``1e-14`` of the largest eigenvalue dropped); Ritz pairs of ``(U^H M U)^-1 U^H A U``; residuals
``||A x - lam M x|| / (||A x|| + |lam| ||M x||)``; stop when every Ritz value inside has converged (with none inside: not before
the second iteration); else ``Y <- U``.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401  (puts the product package on sys.path)

# the regions of the S2k cylinder case (n = 1953): (centre, rx, ry, nodes, subspace), dense count inside, complete
REGIONS = {
    "R1": ((-0.12 + 0.46j, 0.0173, 0.0173, 8, 12), 3, True),
    "R2": ((0.018 + 0.738j, 0.12, 0.12, 16, 48), 13, True),      # the bench shift
    "R0": ((0.45 + 0.0j, 0.46, 1.2, 16, 8), 0, True),            # keeps off the 44-fold Dirichlet lambda = 1
    "R3": ((-0.1 + 0.75j, 0.06, 0.14, 16, 40), 59, False),       # 59 inside, 40 columns: the subspace is too small
}
ATOL = 1e-10
MAX_IT = 12


def start_block(n: int, cols: int, seed: int = 0) -> np.ndarray:
    """The start block of the tests (and ``RegionEigenSolver.start_block``): complex normal from ``default_rng(seed)``."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols))


def nodes_and_weights(centre: complex, rx: float, ry: float, nodes: int):
    t = 2.0 * np.pi * (np.arange(nodes) + 0.5) / nodes
    return centre + rx * np.cos(t) + 1j * ry * np.sin(t), (ry * np.cos(t) + 1j * rx * np.sin(t)) / nodes


def inside(lam, centre: complex, rx: float, ry: float, scale: float = 1.0) -> np.ndarray:
    lam = np.asarray(lam, dtype=np.complex128)
    return ((lam.real - centre.real) / (scale * rx)) ** 2 + ((lam.imag - centre.imag) / (scale * ry)) ** 2 < 1.0


def gram_orth(Q: np.ndarray) -> np.ndarray:
    G = Q.conj().T @ Q
    val, vec = np.linalg.eigh(0.5 * (G + G.conj().T))
    keep = val >= 1e-14 * val.max()
    return Q @ (vec[:, keep] / np.sqrt(val[keep]))


@dataclass
class ReferenceResult:
    eigenvalues: np.ndarray
    eigenvectors: np.ndarray
    residuals: np.ndarray
    count: int
    complete: bool
    estimate: float
    iterations: int
    inside_history: list


def contour_solve(A, M, centre: complex, rx: float, ry: float, nodes: int, Y0: np.ndarray, atol: float = ATOL, max_it: int = MAX_IT) -> ReferenceResult:
    A, M = sp.csr_matrix(A), sp.csr_matrix(M)
    z, w = nodes_and_weights(centre, rx, ry, nodes)
    lus = [spla.splu((A - zk * M).tocsc()) for zk in z]
    Y = np.asarray(Y0, dtype=np.complex128)
    history, stopped, estimate = [], False, 0.0
    for it in range(1, max_it + 1):
        B = M @ Y
        Q = sum(-wk * lu.solve(B) for wk, lu in zip(w, lus))
        if it == 1:
            estimate = float(np.real(np.sum(Y.conj() * Q)) / Y.shape[1])
        U = gram_orth(gram_orth(Q))
        AU, MU = A @ U, M @ U
        lam, S = sla.eig(np.linalg.solve(U.conj().T @ MU, U.conj().T @ AU))
        RA, RM = AU @ S, MU @ S
        res = np.linalg.norm(RA - RM * lam, axis=0) / (np.linalg.norm(RA, axis=0) + np.abs(lam) * np.linalg.norm(RM, axis=0) + 1e-16)
        sel = inside(lam, centre, rx, ry)
        history.append((int(sel.sum()), int(np.sum(res[sel] <= atol))))
        # (an empty region is declared only when a second iteration shows no Ritz value inside either)
        if np.all(res[sel] <= atol) and (sel.any() or it > 1):
            stopped = True
            break
        Y = U
    X = U @ S[:, sel]
    X = X / np.linalg.norm(X, axis=0)
    return ReferenceResult(lam[sel], X, res[sel], int(sel.sum()), bool(stopped and sel.sum() < U.shape[1]), estimate, it, history)


@functools.lru_cache(maxsize=None)
def s2k():
    from synthetic import fem

    es = fem.cylinder_case("S2k")
    return sp.csr_matrix(es.A), sp.csr_matrix(es.M)


@functools.lru_cache(maxsize=None)
def dense_spectrum() -> np.ndarray:
    """The finite eigenvalues of the dense S2k pencil (``scipy.linalg.eig``), without the Dirichlet rows' ``lambda = 1``."""
    A, M = s2k()
    lam = sla.eig(A.toarray(), M.toarray(), right=False)
    lam = lam[np.isfinite(lam)]
    return lam[np.abs(lam - 1.0) > 1e-8]


def match_tolerance(dense: np.ndarray, centre: complex, rx: float, ry: float) -> float:
    """``1e-3 x`` the smallest distance between two distinct dense eigenvalues inside 1.5 radii of the centre (two eigenvalues closer
    than ``1e-9`` count as one)."""
    near = dense[inside(dense, centre, rx, ry, 1.5)]
    if near.size < 2:
        return 1e-3 * min(rx, ry)
    d = np.abs(near[:, None] - near[None, :])
    return 1e-3 * float(d[d > 1e-9].min())


def assert_one_to_one(found: np.ndarray, dense: np.ndarray, region_mask, centre: complex, rx: float, ry: float) -> None:
    """Every found eigenvalue within ``match_tolerance`` of a dense one inside the region, no dense one taken twice, none left over."""
    want = dense[region_mask(dense)]
    assert found.size == want.size, (found.size, want.size)
    if want.size == 0:
        return
    tol = match_tolerance(dense, centre, rx, ry)
    nearest = np.argmin(np.abs(found[:, None] - want[None, :]), axis=1)
    dist = np.abs(found - want[nearest])
    print(f"matching: {found.size} eigenvalues, largest distance {dist.max():.3e}, tolerance {tol:.3e}")
    assert len(set(nearest.tolist())) == want.size and np.all(dist <= tol), (dist.max(), tol)
