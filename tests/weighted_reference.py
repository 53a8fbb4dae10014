"""Host references of the windowed / weighted tests (``test_weighted_cpu.py``, ``test_gpu_weighted.py``): dof coordinates and windows
of the synthetic cylinder pairs, the dense weighted gains, a numpy restatement of the library's weighted resolvent iteration and the
transient-growth march with the response weight at its turn.  Conventions (``resolvent_reference.py``, ``growth_reference.py``):
``R = (s M - A)^-1 = -C^-1`` with ``C = A - s M`` at the complex shift ``s = beta + i omega``; with a forcing weight ``Qf`` and a response
weight ``Qq`` the response is ``q = R Qf f``, the gains are ``max ||q||_Qq / ||f||_Qf`` and ``sigma^2`` are the non-zero eigenvalues of
``W = C^-1 Qf C^-H Qq``.  For transient growth only the response is weighted: ``W = M^-1 Phi^T Q Phi``."""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401
import growth_reference as gref
import growth_sdirk_reference as sref
import resolvent_reference as rref
from resolvent_reference import OMEGA_TARGET, case

OMEGA_F = (-3.0, 3.0, -3.0, 3.0)  # the forcing region x0, x1, y0, y1: 90 velocity dofs with mass on S2k
OMEGA_Q = (2.0, 30.0)  # the response region x0, x1
NEAR = (0.0, 20.0)  # "response x in [0, 20] only"
BETA = 0.1

# dense gains, six decimals (S2k, Re = 50), by (beta, omega, forcing region, response region)
GAINS = {
    (0.0, OMEGA_TARGET, None, NEAR): (26.259250, 23.793029, 23.376688, 22.056971),
    (0.0, OMEGA_TARGET, OMEGA_F, OMEGA_Q): (17.093709, 8.420070, 7.661445, 4.941163),
    (0.0, 0.4, OMEGA_F, OMEGA_Q): (39.586842, 14.756616, 9.429739, 6.147641),
    (BETA, OMEGA_TARGET, OMEGA_F, OMEGA_Q): (6.482421, 4.013982, 3.729233, 2.732792),
    (BETA, OMEGA_TARGET, None, None): (9.677390, 8.101018, 8.085360, 7.964364),
}
GAINS_REAL_SHIFT = (5.641285, 5.041370)  # z = 0.2, no windows
# windowed growth (Euler, dt = 0.25, response x in [2, 30]), by N
GROWTH_GAINS = {16: (1.686490, 1.541267, 1.266960), 40: (3.070572, 2.610745, 1.715178)}


@functools.lru_cache(maxsize=None)
def dof_xy(name: str) -> tuple[np.ndarray, np.ndarray]:
    """(x, y) of every dof of a synthetic cylinder case: a node's two velocity dofs and, on a vertex, its pressure dof sit at the
    node (``mesh.node_xy()``, ``node_offset``)."""
    from synthetic import fem

    es = fem.cylinder_case(name)
    X, Y = es.mesh.node_xy()
    isv = es.mesh.is_vertex()
    off = np.asarray(es.node_offset)
    x, y = np.full(es.n, np.nan), np.full(es.n, np.nan)
    for c in (0, 1):
        x[off + c], y[off + c] = X, Y
    x[off[isv] + 2], y[off[isv] + 2] = X[isv], Y[isv]
    assert not np.isnan(x).any()
    return x, y


def window(name: str, x0: float, x1: float, y0: float = -np.inf, y1: float = np.inf) -> np.ndarray:
    """The 0/1 window of the dofs with ``x0 <= x <= x1`` and ``y0 <= y <= y1``."""
    x, y = dof_xy(name)
    return ((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)).astype(np.float64)


def region(name: str, box) -> np.ndarray | None:
    return None if box is None else window(name, *box)


def weighted(M, left, right=None) -> sp.csr_matrix:
    """``diag(left) M diag(right)`` on ``M``'s pattern, entry by entry ``(left[i] * m_ij) * right[j]``: the roundings of
    ``scipy.sparse.diags(left) @ M @ scipy.sparse.diags(right)`` and of ``lsa_csr_window``."""
    M = sp.csr_matrix(M)
    right = left if right is None else right
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    data = (np.asarray(left, dtype=np.float64)[rows] * M.data) * np.asarray(right, dtype=np.float64)[M.indices]
    return sp.csr_matrix((data, M.indices.copy(), M.indptr.copy()), shape=M.shape)


def weight_of(name: str, box):
    """The weight of a region: ``M`` itself for ``None``."""
    _, M = case(name)
    return M if box is None else weighted(M, window(name, *box))


@functools.lru_cache(maxsize=None)
def _sqrt_of(name: str, box) -> np.ndarray:
    """The symmetric square root of a region's weight through ``eigh`` (negative rounding-level eigenvalues clipped, as
    ``resolvent_reference.dense_gains_svd`` does)."""
    d, U = np.linalg.eigh(weight_of(name, box).toarray())
    return (U * np.sqrt(np.clip(d, 0.0, None))) @ U.T


@functools.lru_cache(maxsize=None)
def dense_gains(name: str, beta: float, omega: float, fbox=None, qbox=None) -> np.ndarray:
    """All gains, descending: the singular values of ``Qq^(1/2) C^-1 Qf^(1/2)`` at the shift ``beta + i omega``."""
    A, M = case(name)
    C = (A - complex(beta, omega) * M).toarray().astype(np.complex128)
    return np.linalg.svd(_sqrt_of(name, qbox) @ np.linalg.solve(C, _sqrt_of(name, fbox).astype(np.complex128)), compute_uv=False)


class HostWeighted:
    """``C^-1``, ``C^-H`` and ``W = C^-1 Qf C^-H Qq`` applied on the host by SuperLU at a complex shift."""

    def __init__(self, A, M, shift, Qf=None, Qq=None):
        self.M = sp.csr_matrix(M)
        self.Qf = self.M if Qf is None else sp.csr_matrix(Qf)
        self.Qq = self.M if Qq is None else sp.csr_matrix(Qq)
        self.lu = spla.splu((A - complex(shift) * M).tocsc().astype(np.complex128))

    def _cols(self, b, trans):
        b = np.asarray(b, dtype=np.complex128)
        return self.lu.solve(b, trans=trans) if b.ndim == 1 else np.column_stack([self.lu.solve(b[:, c], trans=trans) for c in range(b.shape[1])])

    def solve(self, b):
        return self._cols(b, "N")

    def solve_h(self, b):
        return self._cols(b, "H")

    def W(self, v):
        return self.solve(self.Qf @ self.solve_h(self.Qq @ v))

    def R(self, v):
        return -self.solve(v)


def resolvent_trl(A, M, shift, nev, ncv, tol, v0, Qf=None, Qq=None, keep_fraction=0.5, max_restarts=200):
    """``resolvent_reference.resolvent_trl`` with the weights in the three places ``M`` stands there: Lanczos on ``W`` in the
    ``Qq``-semi-inner product (``rhs = Qq v``, ``tm = Qf z``, ``t = Qq w``), the forcings ``f_j = -C^-H Qq q_j / sigma_j``.  Returns the
    same dict."""
    host = HostWeighted(A, M, shift, Qf, Qq)
    Q = host.Qq
    n, m = A.shape[0], int(ncv)
    V = np.zeros((n, m + 1), dtype=np.complex128)
    T = np.zeros((m + 1, m))

    def orth(w, j):
        h = np.zeros(j, dtype=np.complex128)
        for _ in range(2):
            c = V[:, :j].conj().T @ (Q @ w)
            w = w - V[:, :j] @ c
            h += c
        return w, h, float((w.conj() @ (Q @ w)).real)

    w, _, b2 = orth(np.asarray(v0, dtype=np.complex128), 0)
    V[:, 0] = w / np.sqrt(b2)
    kept = restarts = applies = 0
    while True:
        for j in range(kept, m):
            w, h, b2 = orth(host.W(V[:, j]), j + 1)
            applies += 1
            alpha, beta = h[j].real, np.sqrt(b2)
            T[j, j] = alpha
            T[j + 1, j] = beta
            if j + 1 < m:
                T[j, j + 1] = beta
            V[:, j + 1] = w / beta
        theta, Y = np.linalg.eigh(T[:m, :m])
        beta = T[m, m - 1]
        rel = np.abs(beta * Y[m - 1, :]) / np.abs(theta)
        order = np.argsort(-theta, kind="stable")
        nconv = 0
        while nconv < m and rel[order[nconv]] <= tol:
            nconv += 1
        if nconv >= nev or restarts >= max_restarts:
            break
        knew = max(min(nconv + int((m - nconv) * keep_fraction), m - 1), 1)
        sel = order[:knew]
        last = V[:, m].copy()
        V[:, :knew] = V[:, :m] @ Y[:, sel]
        V[:, knew] = last
        T[:] = 0.0
        T[np.arange(knew), np.arange(knew)] = theta[sel]
        T[knew, :knew] = T[:knew, knew] = beta * Y[m - 1, sel]
        kept = knew
        restarts += 1
    k = min(nconv, nev)
    sel = order[:k]
    gains = np.sqrt(theta[sel])
    Qv = np.column_stack([rref.canonical(q) for q in (V[:, :m] @ Y[:, sel]).T]) if k else np.zeros((n, 0), dtype=np.complex128)
    F = -host.solve_h(Q @ Qv) / gains if k else Qv
    return {"gains": gains, "Q": Qv, "F": F, "restarts": restarts, "applies": applies, "T": T.copy(), "estimates": rel[sel]}


def pair_checks(A, M, shift, gains, Q, F, Qf=None, Qq=None):
    """(``||Q^H Qq Q - I||_max``, ``||F^H Qf F - I||_max``, ``max_j ||R Qf f_j - sigma_j q_j||_Qq / sigma_j``), ``R`` applied by SuperLU."""
    host = HostWeighted(A, M, shift, Qf, Qq)
    k = Q.shape[1]
    oq = np.abs(Q.conj().T @ (host.Qq @ Q) - np.eye(k)).max()
    of = np.abs(F.conj().T @ (host.Qf @ F) - np.eye(k)).max()
    D = host.R(host.Qf @ F) - Q * gains
    return float(oq), float(of), float((rref.m_norm_columns(host.Qq, D) / gains).max())


# ---- transient growth with a response weight ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_growth_gains(name: str, nsteps: int, qbox) -> np.ndarray:
    """All gains of the implicit-Euler march at ``growth_reference.DT``, descending: ``Phi = Xi M`` as in
    ``growth_reference.dense_gains``, so the gains ``max ||Phi q||_Q^2 / ||q||_M^2`` are the squared singular values of
    ``Q^(1/2) Xi M^(1/2)`` on the free dofs."""
    S, Md, Cinv = gref._dense_step(name)
    f = np.flatnonzero(gref.keep_mask(name) == 1.0)
    d, U = np.linalg.eigh(weight_of(name, qbox).toarray()[np.ix_(f, f)])
    Sq = (U * np.sqrt(np.clip(d, 0.0, None))) @ U.T
    sigma = 1.0 / gref.DT
    P = -sigma * (Cinv @ Md)
    Xi = -sigma * (np.linalg.matrix_power(P, nsteps - 1) @ Cinv)
    return np.linalg.svd(Sq @ Xi @ S, compute_uv=False) ** 2


class TurnedMarch:
    """A host march (``growth_reference.HostMarch`` or ``growth_sdirk_reference.SdirkMarch``) with the response weight ``Q`` at the
    turn of ``W``: ``N`` forward time steps, the first transposed solve on ``-sigma keep (.) (Q x)`` instead of ``-sigma keep (.) (M x)``
    (under SDIRK2 the combining stage after it reads that same vector), then the rest of the transposed march.  ``M``, ``keep``,
    ``march`` and ``energy`` are the wrapped march's: what ``growth_sdirk_reference.march_trl`` asks of a host."""

    def __init__(self, host, Q):
        self.host, self.Q = host, sp.csr_matrix(Q)
        self.M, self.keep = host.M, host.keep

    def W(self, v, nsteps):
        h = self.host
        x = np.asarray(v, dtype=np.float64)
        for _ in range(nsteps):
            x = h.step(x)
        u = -h.sigma * h.keep * h.lu.solve(self.Q @ x, trans="T")  # S+ M^-1 Q x
        x = gref.HostMarch.step(h, sref.A2 * u, "T") + sref.B2 * u if isinstance(h, sref.SdirkMarch) else u
        for _ in range(nsteps - 1):
            x = h.step(x, "T")
        return x

    def march(self, q, nsteps):
        return self.host.march(q, nsteps)

    def energy(self, X):
        return self.host.energy(X)

    def response_energy(self, X):
        return np.einsum("ic,ic->c", X, self.Q @ X)
