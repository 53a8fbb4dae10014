"""Host references of the resolvent tests (``test_resolvent_cpu.py``, ``test_gpu_resolvent.py``): the synthetic cylinder pairs, two
dense routes to the optimal gains, and a numpy restatement of the library's iteration (``csrc/resolvent.hip`` + the loop of
``lsa_lanczos_solve``).  Conventions: ``A x = lambda M x``, ``R = (i omega M - A)^-1 = -C^-1`` with ``C = A - i omega M``; the gains are
the square roots of the largest eigenvalues of ``W = R M R^H M = C^-1 M C^-H M``."""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401

OMEGA_TARGET = 0.7379601143282424  # the imaginary part of the Re = 50 eigenvalue target
OMEGAS = (0.0, 0.4, OMEGA_TARGET)

# dense gains, six decimals (S2k: n = 1953, S5k: n = 4851; Re = 50)
GAINS_S2K = {
    OMEGA_TARGET: (27.711306, 26.685607, 26.313727, 24.766504),
    0.4: (90.719699, 56.104099, 54.174743, 50.028159),
    0.0: (117.678034, 103.823501, 103.155428, 101.207390),
}
GAINS_S5K = (53.038619, 37.038706, 36.205045, 33.798558, 33.623103, 32.025501)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(A, M) of a synthetic cylinder case as CSR matrices."""
    from synthetic import fem

    es = fem.cylinder_case(name)
    return sp.csr_matrix(es.A), sp.csr_matrix(es.M)


def shifted(A, M, omega):
    return (A - 1j * omega * M).tocsc().astype(np.complex128)


@functools.lru_cache(maxsize=None)
def dense_gains_svd(name: str, omega: float) -> np.ndarray:
    """All gains, descending: the singular values of ``M^(1/2) C^-1 M^(1/2)``, the square root through ``eigh(M)`` (negative
    rounding-level eigenvalues of the semidefinite ``M`` clipped)."""
    A, M = case(name)
    d, U = np.linalg.eigh(M.toarray())
    S = (U * np.sqrt(np.clip(d, 0.0, None))) @ U.T
    X = np.linalg.solve(shifted(A, M, omega).toarray(), S)
    return np.linalg.svd(S @ X, compute_uv=False)


@functools.lru_cache(maxsize=None)
def dense_gains_eig(name: str, omega: float) -> np.ndarray:
    """All gains, descending: the square roots of the eigenvalues of ``W = C^-1 M C^-H M``."""
    A, M = case(name)
    Md = M.toarray()
    Cd = shifted(A, M, omega).toarray()
    W = np.linalg.solve(Cd, Md @ np.linalg.solve(Cd.conj().T, Md.astype(np.complex128)))
    ev = np.linalg.eigvals(W)
    return np.sqrt(np.clip(np.sort(ev.real)[::-1], 0.0, None))


class HostResolvent:
    """``C^-1``, ``C^-H`` and ``W`` applied on the host by SuperLU."""

    def __init__(self, A, M, omega):
        self.M = sp.csr_matrix(M)
        self.lu = spla.splu(shifted(A, M, omega))

    def solve(self, b):
        return self._cols(b, "N")

    def solve_h(self, b):
        return self._cols(b, "H")

    def _cols(self, b, trans):
        b = np.asarray(b, dtype=np.complex128)
        return self.lu.solve(b, trans=trans) if b.ndim == 1 else np.column_stack([self.lu.solve(b[:, c], trans=trans) for c in range(b.shape[1])])

    def W(self, v):
        return self.solve(self.M @ self.solve_h(self.M @ v))

    def R(self, v):  # R = (i omega M - A)^-1
        return -self.solve(v)


def m_norm_columns(M, X):
    """``sqrt(x_c^H M x_c)`` per column."""
    return np.sqrt(np.clip(np.einsum("ic,ic->c", X.conj(), M @ X).real, 0.0, None))


def canonical(x):
    k = int(np.argmax(np.abs(x)))
    return x * (np.conj(x[k]) / abs(x[k]))


def resolvent_trl(A, M, omega, nev, ncv, tol, v0, keep_fraction=0.5, max_restarts=100):
    """The library's iteration restated: Lanczos on ``W`` in the ``M``-inner product with a complex basis and two passes of classical
    Gram-Schmidt, ``alpha_j = Re h_j``, a real projected matrix, thick restart with the real eigenvectors of it (kept: the converged
    ones and ``keep_fraction`` of the rest), Ritz values ranked largest first and accepted on ``|beta y_mi| / theta_i <= tol``.
    Returns a dict: ``gains``, ``Q``, ``F``, ``restarts``, ``applies``, ``T`` (the last projected matrix, (m+1) x m), ``imag_ratio``
    (``max |Im h_j| / |alpha_j|``)."""
    host = HostResolvent(A, M, omega)
    M = host.M
    n, m = A.shape[0], int(ncv)
    V = np.zeros((n, m + 1), dtype=np.complex128)
    T = np.zeros((m + 1, m))

    def orth(w, j):
        h = np.zeros(j, dtype=np.complex128)
        for _ in range(2):
            c = V[:, :j].conj().T @ (M @ w)
            w = w - V[:, :j] @ c
            h += c
        return w, h, float((w.conj() @ (M @ w)).real)

    w, _, b2 = orth(np.asarray(v0, dtype=np.complex128), 0)
    V[:, 0] = w / np.sqrt(b2)
    kept = restarts = applies = 0
    imag_ratio = 0.0
    while True:
        for j in range(kept, m):
            w, h, b2 = orth(host.W(V[:, j]), j + 1)
            applies += 1
            alpha, beta = h[j].real, np.sqrt(b2)
            imag_ratio = max(imag_ratio, abs(h[j].imag) / abs(alpha))
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
    Q = np.column_stack([canonical(q) for q in (V[:, :m] @ Y[:, sel]).T]) if k else np.zeros((n, 0), dtype=np.complex128)
    F = -host.solve_h(M @ Q) / gains if k else Q
    return {"gains": gains, "Q": Q, "F": F, "restarts": restarts, "applies": applies, "T": T.copy(), "imag_ratio": imag_ratio, "estimates": rel[sel]}


def pair_checks(A, M, omega, gains, Q, F):
    """(``||Q^H M Q - I||_max``, ``||F^H M F - I||_max``, ``max_j ||R M f_j - sigma_j q_j||_M / sigma_j``), ``R`` applied by SuperLU."""
    host = HostResolvent(A, M, omega)
    M = host.M
    k = Q.shape[1]
    oq = np.abs(Q.conj().T @ (M @ Q) - np.eye(k)).max()
    of = np.abs(F.conj().T @ (M @ F) - np.eye(k)).max()
    D = host.R(M @ F) - Q * gains
    return float(oq), float(of), float((m_norm_columns(M, D) / gains).max())


def start_vector(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)
