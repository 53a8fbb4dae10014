"""Host references of the stochastic-forcing tests (``test_stochastic_cpu.py``, ``test_gpu_stochastic.py``): the quadrature rules, the
quadrature operator applied through SuperLU factors per node, a dense form of it, the Lyapunov pair, and a numpy restatement of the
library's iteration (``csrc/stochastic.hip`` + the loop of ``lsa_lanczos_solve``).  Conventions (``weighted_reference.py``):
``C_k = A - z_k M`` at ``z_k = beta + i omega_k``, ``W(z) = C^-1 Qf C^-H Qq``; the EOF operator is ``S = (1 / pi) sum_k w_k Re W(z_k)``,
self-adjoint in ``Qq``; the operator of the stochastic optimals is ``S' = (1 / pi) sum_k w_k Re(C_k^-H Qq C_k^-1 Qf)``, self-adjoint in
``Qf``."""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import helpers  # noqa: F401
from resolvent_reference import case  # noqa: F401
from weighted_reference import HostWeighted

BAND = (0.0, 1.5)
# S2k (n = 1953, Re = 50), band [0, 1.5], 8 Gauss nodes: the four largest eigenvalues of the EOF operator, six decimals (ARPACK)
VARIANCES_S2K_8 = (460.938143, 446.137113, 364.773091, 362.060362)


def gauss_band(a, b, N):
    """Gauss-Legendre on ``[a, b]``."""
    x, w = np.polynomial.legendre.leggauss(N)
    return 0.5 * (b - a) * x + 0.5 * (a + b), 0.5 * (b - a) * w


def tan_rule(s, N):
    """``[0, inf)`` under ``omega = s tan(theta)``: Gauss-Legendre in ``theta`` on ``[0, pi / 2]``."""
    th, w = gauss_band(0.0, 0.5 * np.pi, N)
    return s * np.tan(th), s * w / np.cos(th) ** 2


class HostStochastic:
    """The quadrature operator of both kinds applied on the host: one SuperLU factorisation per node (``HostWeighted``)."""

    def __init__(self, A, M, omegas, weights, Qf=None, Qq=None, discount=0.0, permc_spec="COLAMD"):
        import scipy.sparse.linalg as spla

        self.omegas, self.weights = np.asarray(omegas, dtype=float), np.asarray(weights, dtype=float)
        self.nodes = [HostWeighted(A, M, complex(discount, om), Qf, Qq) for om in self.omegas]
        if permc_spec != "COLAMD":
            for h, om in zip(self.nodes, self.omegas):
                h.lu = spla.splu((A - complex(discount, om) * M).tocsc().astype(np.complex128), permc_spec=permc_spec)
        self.Qf, self.Qq = self.nodes[0].Qf, self.nodes[0].Qq

    def weight(self, kind):
        """The inner product of a kind."""
        return self.Qq if kind == "eofs" else self.Qf

    def node_vectors(self, v, kind="eofs"):
        """``Re W_k v`` per node (``n x N``), ``W_k`` the node's operator of the kind."""
        v = np.asarray(v, dtype=float)
        cols = []
        for h in self.nodes:
            if kind == "eofs":
                cols.append(h.solve(h.Qf @ h.solve_h(h.Qq @ v)).real)
            else:
                cols.append(h.solve_h(h.Qq @ h.solve(h.Qf @ v)).real)
        return np.column_stack(cols)

    def apply(self, v, kind="eofs"):
        """``(S v, node terms)``: the terms are ``(w_k / pi) (Q v)^T Re W_k v`` and sum to ``v^T Q S v``."""
        R = self.node_vectors(v, kind)
        c = self.weights / np.pi
        return R @ c, c * ((self.weight(kind) @ np.asarray(v, dtype=float)) @ R)


def dense_operator(A, M, omegas, weights, Qf=None, Qq=None, discount=0.0, kind="eofs"):
    """The quadrature operator as a dense real matrix."""
    Ad, Md = A.toarray(), M.toarray()
    Qf = Md if Qf is None else sp.csr_matrix(Qf).toarray()
    Qq = Md if Qq is None else sp.csr_matrix(Qq).toarray()
    S = np.zeros_like(Ad)
    for om, w in zip(omegas, weights):
        C = Ad - complex(discount, om) * Md
        if kind == "eofs":
            S += (w / np.pi) * np.linalg.solve(C, Qf @ np.linalg.solve(C.conj().T, Qq.astype(complex))).real
        else:
            S += (w / np.pi) * np.linalg.solve(C.conj().T, Qq @ np.linalg.solve(C, Qf.astype(complex))).real
    return S


@functools.lru_cache(maxsize=None)
def dense_variances_s2k(N=8):
    """All eigenvalues of the EOF operator of S2k on ``BAND`` with ``N`` Gauss nodes, descending (about 20 s: once per session)."""
    A, M = case("S2k")
    om, w = gauss_band(*BAND, N)
    ev = np.linalg.eigvals(dense_operator(A, M, om, w))
    return np.sort(ev.real)[::-1]


LYAPUNOV_SCALE = 1.0  # s of omega = s tan(theta) for the Lyapunov pair: its eigenvalues lie in -4.3 <= Re <= -1.4, |Im| <= 2.4


def lyapunov_pair(n=40, seed=0):
    """A seeded dense stable pair with SPD ``M``: ``M^-1 A = -(I + G G^T / n) + (K - K^T) / sqrt(n)``, a symmetric part below ``-1``
    and a skew part, so every eigenvalue has a real part below ``-1``."""
    rng = np.random.default_rng(seed)
    G, K, L = rng.standard_normal((n, n)), rng.standard_normal((n, n)), rng.standard_normal((n, n))
    M = L @ L.T / n + np.eye(n)
    A = M @ (-(np.eye(n) + G @ G.T / n) + (K - K.T) / np.sqrt(n))
    return A, M


def lyapunov_variances(A, M, k=4):
    """The ``k`` largest eigenvalues of ``P M`` with ``P`` the response covariance of ``M q' = A q + f`` under white forcing with
    weight ``Qf = M``: ``q' = F q + M^-1 f``, so ``F P + P F^T + M^-1 M M^-1 = 0`` with ``F = M^-1 A``."""
    from scipy.linalg import solve_continuous_lyapunov

    Minv = np.linalg.inv(M)
    P = solve_continuous_lyapunov(Minv @ A, -Minv)
    return np.sort(np.linalg.eigvals(P @ M).real)[::-1][:k]


def canonical(x):
    k = int(np.argmax(np.abs(x)))
    return x if x[k] > 0 else -x


def stochastic_trl(host, kind, nev, ncv, tol, v0, keep_fraction=0.5, max_restarts=200):
    """The library's iteration restated (``resolvent_reference.resolvent_trl`` with real vectors): Lanczos on the quadrature operator
    of ``host`` in the kind's weight with two passes of classical Gram-Schmidt, thick restart with the eigenvectors of the projected
    matrix (kept: the converged ones and ``keep_fraction`` of the rest), Ritz values ranked largest first and accepted on
    ``|beta y_mi| / theta_i <= tol``.  Returns a dict: ``variances``, ``modes``, ``restarts``, ``applies``, ``estimates``."""
    Q = host.weight(kind)
    n, m = Q.shape[0], int(ncv)
    V = np.zeros((n, m + 1))
    T = np.zeros((m + 1, m))

    def orth(w, j):
        h = np.zeros(j)
        for _ in range(2):
            c = V[:, :j].T @ (Q @ w)
            w = w - V[:, :j] @ c
            h += c
        return w, h, float(w @ (Q @ w))

    w, _, b2 = orth(np.asarray(v0, dtype=float), 0)
    V[:, 0] = w / np.sqrt(b2)
    kept = restarts = applies = 0
    while True:
        for j in range(kept, m):
            w, h, b2 = orth(host.apply(V[:, j], kind)[0], j + 1)
            applies += 1
            alpha, beta = h[j], np.sqrt(b2)
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
    X = np.column_stack([canonical(x) for x in (V[:, :m] @ Y[:, sel]).T]) if k else np.zeros((n, 0))
    return {"variances": theta[sel], "modes": X, "restarts": restarts, "applies": applies, "estimates": rel[sel]}


def weight_norm(Q, x):
    return float(np.sqrt(max(x @ (Q @ x), 0.0)))
