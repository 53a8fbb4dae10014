"""Host references of the transient-growth tests (``test_growth_cpu.py``, ``test_gpu_growth.py``): the synthetic cylinder pairs, the
dense optimal gains, a SuperLU march and a numpy restatement of the library's masked iteration (``csrc/growth.hip`` + the loop of
``lsa_lanczos_solve``).  Conventions: ``M q' = A q``; one implicit-Euler step is ``q+ = -sigma C^-1 M q`` with ``C = A - sigma M`` and
``sigma = 1 / dt``; ``Phi = (-sigma C^-1 M)^N``, ``Phi+ = (-sigma C^-T M)^N`` and the gains are the largest eigenvalues of
``W = Phi+ Phi`` on the free dofs."""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401
from resolvent_reference import case  # noqa: F401  (the same synthetic pairs, cached once for both suites)

DT = 0.25

# dense gains, six decimals (S2k: n = 1953, 44 constrained rows; S5k: n = 4851, 71 constrained rows; Re = 50, dt = 0.25)
GAINS = {
    ("S2k", 16): (2.230737, 1.751372, 1.496285),
    ("S2k", 40): (3.247074, 2.736523, 1.887518),
    ("S2k", 80): (3.451581, 3.297204),
    ("S5k", 16): (3.048769, 2.449263, 2.349194, 1.960534),
}
CONSTRAINED = {"S2k": 44, "S5k": 71}
SPURIOUS_S2K_N16 = 0.75 ** -32  # the unmasked boundary mode lambda = 1: (1 - dt)^(-2 N)


def decoupled_rows(A, M) -> np.ndarray:
    """Indices whose row and column hold no off-diagonal non-zero in both ``A`` and ``M`` (the front end's ``"auto"`` rule, restated)."""
    n = A.shape[0]
    free = np.zeros(n, dtype=bool)
    for X in (A, M):
        C = sp.coo_matrix(X)
        off = (C.row != C.col) & (C.data != 0)
        free[C.row[off]] = True
        free[C.col[off]] = True
    return np.flatnonzero(~free)


@functools.lru_cache(maxsize=None)
def keep_mask(name: str) -> np.ndarray:
    A, M = case(name)
    keep = np.ones(A.shape[0])
    keep[decoupled_rows(A, M)] = 0.0
    return keep


@functools.lru_cache(maxsize=None)
def _dense_step(name: str):
    """(S, X): the symmetric square root of ``M`` on the free dofs (negative rounding-level eigenvalues of the semidefinite ``M``
    clipped) and ``C^-1`` there, dense."""
    A, M = case(name)
    f = np.flatnonzero(keep_mask(name) == 1.0)
    Ad, Md = A.toarray()[np.ix_(f, f)], M.toarray()[np.ix_(f, f)]
    d, U = np.linalg.eigh(Md)
    S = (U * np.sqrt(np.clip(d, 0.0, None))) @ U.T
    return S, Md, np.linalg.inv(Ad - Md / DT)


@functools.lru_cache(maxsize=None)
def dense_gains(name: str, nsteps: int) -> np.ndarray:
    """All gains, descending.  ``Phi = Xi M`` with ``Xi = -sigma (-sigma C^-1 M)^(N-1) C^-1``, so the non-zero eigenvalues of
    ``Phi+ Phi = Xi^T M Xi M`` are those of ``(S Xi S)^T (S Xi S)``, ``S = M^(1/2)``: the squared singular values of ``S Xi S``."""
    S, Md, Cinv = _dense_step(name)
    sigma = 1.0 / DT
    P = -sigma * (Cinv @ Md)
    Xi = -sigma * (np.linalg.matrix_power(P, nsteps - 1) @ Cinv)
    return np.linalg.svd(S @ Xi @ S, compute_uv=False) ** 2


class HostMarch:
    """``C^-1``, ``C^-T``, the masked step and ``W`` applied on the host by SuperLU."""

    def __init__(self, A, M, dt=DT, keep=None):
        self.M = sp.csr_matrix(M)
        self.sigma = 1.0 / dt
        self.keep = np.ones(A.shape[0]) if keep is None else np.asarray(keep, dtype=np.float64)
        self.lu = spla.splu((A - self.sigma * M).tocsc().astype(np.float64))

    def step(self, q, trans="N"):
        """One implicit-Euler step (``trans="T"``: of the adjoint march)."""
        return -self.sigma * self.keep * self.lu.solve(self.M @ q, trans=trans)

    def march(self, q, nsteps):
        """``[q, Phi_1 q, ..., Phi_N q]`` as columns."""
        out = [np.asarray(q, dtype=np.float64)]
        for _ in range(nsteps):
            out.append(self.step(out[-1]))
        return np.column_stack(out)

    def W(self, v, nsteps):
        x = np.asarray(v, dtype=np.float64)
        for _ in range(nsteps):
            x = self.step(x)
        for _ in range(nsteps):
            x = self.step(x, "T")
        return x

    def energy(self, Q):
        return np.einsum("ic,ic->c", Q, self.M @ Q)


def growth_trl(A, M, dt, nsteps, keep, nev, ncv, tol, v0, keep_fraction=0.5, max_restarts=100):
    """The library's iteration restated: Lanczos on ``W`` in the ``M``-inner product with a real basis and two passes of classical
    Gram-Schmidt, every right-hand side of the march and the start vector multiplied by ``keep``, thick restart with the eigenvectors
    of the projected matrix (kept: the converged ones and ``keep_fraction`` of the rest), Ritz values ranked largest first and accepted
    on ``|beta y_mi| / theta_i <= tol``.  Returns a dict: ``gains``, ``Q0``, ``restarts``, ``applies``, ``T``, ``estimates``."""
    host = HostMarch(A, M, dt, keep)
    M = host.M
    n, m = A.shape[0], int(ncv)
    V = np.zeros((n, m + 1))
    T = np.zeros((m + 1, m))

    def orth(w, j):
        h = np.zeros(j)
        for _ in range(2):
            c = V[:, :j].T @ (M @ w)
            w = w - V[:, :j] @ c
            h += c
        return w, h, float(w @ (M @ w))

    w, _, b2 = orth(host.keep * np.asarray(v0, dtype=np.float64), 0)
    V[:, 0] = w / np.sqrt(b2)
    kept = restarts = applies = 0
    while True:
        for j in range(kept, m):
            w, h, b2 = orth(host.W(V[:, j], nsteps), j + 1)
            applies += 1
            beta = np.sqrt(b2)
            T[j, j] = h[j]
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
    Q0 = V[:, :m] @ Y[:, sel]
    for c in range(k):
        Q0[:, c] *= np.sign(Q0[int(np.argmax(np.abs(Q0[:, c]))), c])
    return {"gains": theta[sel], "Q0": Q0, "restarts": restarts, "applies": applies, "T": T.copy(), "estimates": rel[sel]}


def start_vector(n: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal(n)
