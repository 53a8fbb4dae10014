"""Host references of the SDIRK2 transient-growth tests (``test_growth_sdirk_cpu.py``, ``test_gpu_growth_sdirk.py``), beside those of
``growth_reference.py`` for implicit Euler: the dense optimal gains, a SuperLU march and the numpy restatement of the library's masked
iteration on it.  The scheme is the L-stable, stiffly accurate two-stage SDIRK method with ``gamma = 1 - 1/sqrt(2)``: both stages solve
with ``M - gamma dt A``, i.e. ``C = A - sigma M`` at ``sigma = 1 / (gamma dt)``, and with ``S = -sigma C^-1 M`` one time step is
``Phi_1 = S (a S + b I)``, ``a = 1 + sqrt(2)``, ``b = -sqrt(2)``: the stability function ``(1 + (1 - 2 gamma) z) / (1 - gamma z)^2``
written in ``s = 1 / (1 - gamma z)``.  ``Phi = Phi_1^N``, its ``M``-adjoint is the same with ``C^-T``, the gains are the largest
eigenvalues of ``W = Phi+ Phi`` on the free dofs."""

from __future__ import annotations

import functools

import numpy as np

import helpers  # noqa: F401
import growth_reference as ref

GAMMA = 1.0 - 1.0 / np.sqrt(2.0)
A2, B2 = 1.0 + np.sqrt(2.0), -np.sqrt(2.0)
DT = 0.5

# dense gains, six decimals (S2k, Re = 50), by (dt, N)
GAINS = {
    (0.5, 8): (2.548908, 2.127805, 1.835609),
    (0.5, 20): (4.290110, 3.940617, 2.617808),
    (0.25, 16): (2.553968, 2.135460, 1.840648),
}


@functools.lru_cache(maxsize=None)
def dense_gains(name: str, dt: float, nsteps: int, scheme: str = "sdirk2") -> np.ndarray:
    """All gains, descending, the way ``growth_reference.dense_gains`` takes them: ``Phi = Xi M`` with
    ``Xi = Phi_1^(N-1) (a P + b I) (-sigma C^-1)`` and ``P = -sigma C^-1 M``, so the gains are the squared singular values of ``S Xi S``,
    ``S = M^(1/2)`` on the free dofs.  ``scheme="euler"``: ``gamma = 1``, ``a = 0``, ``b = 1``, that module's formula at any ``dt``."""
    gamma, a, b = {"sdirk2": (GAMMA, A2, B2), "euler": (1.0, 0.0, 1.0)}[scheme]
    A, M = ref.case(name)
    f = np.flatnonzero(ref.keep_mask(name) == 1.0)
    S, Md, _ = ref._dense_step(name)  # (the square root of M does not depend on the step)
    sigma = 1.0 / (gamma * dt)
    Cinv = np.linalg.inv(A.toarray()[np.ix_(f, f)] - sigma * Md)
    P = -sigma * (Cinv @ Md)
    stage = a * P + b * np.eye(f.size)
    Xi = np.linalg.matrix_power(P @ stage, nsteps - 1) @ stage @ (-sigma * Cinv)
    return np.linalg.svd(S @ Xi @ S, compute_uv=False) ** 2


class SdirkMarch(ref.HostMarch):
    """``growth_reference.HostMarch`` built at ``gamma dt`` with the two-stage time step; ``march``, ``W`` and ``energy`` come along."""

    def __init__(self, A, M, dt=DT, keep=None):
        super().__init__(A, M, GAMMA * dt, keep)
        self.dt = dt

    def step(self, q, trans="N"):
        """One SDIRK2 time step ``S (a S + b I) q`` (``trans="T"``: of the adjoint march, ``S+ (a S+ + b I) q``)."""
        base = super().step
        return base(A2 * base(q, trans) + B2 * np.asarray(q, dtype=np.float64), trans)


def march_trl(host, nsteps, nev, ncv, tol, v0, keep_fraction=0.5, max_restarts=100):
    """The loop of ``growth_reference.growth_trl`` with the march handed in (that function builds its own ``HostMarch``): Lanczos on
    ``host.W`` in the ``M``-inner product, two passes of classical Gram-Schmidt, the start vector multiplied by ``host.keep``, thick
    restart on the eigenvectors of the projected matrix, Ritz values largest first, accepted on ``|beta y_mi| / theta_i <= tol``."""
    M = host.M
    n, m = M.shape[0], int(ncv)
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


def sdirk_trl(name, dt, nsteps, nev, ncv, tol, v0):
    """The library's SDIRK2 iteration restated for a named case."""
    A, M = ref.case(name)
    return march_trl(SdirkMarch(A, M, dt, ref.keep_mask(name)), nsteps, nev, ncv, tol, v0)
