"""Host references of the trace tests (``test_stochastic_trace_cpu.py``, ``test_gpu_stochastic_trace.py``): a numpy restatement of the
probe generator of ``csrc/stochastic_trace.hip`` and of its two-column estimator on the SuperLU nodes of
``stochastic_reference.HostStochastic``.

For a real probe ``z`` and ``p = z - U (U^T Q z)`` (``Q`` the kind's weight, ``U`` modes orthonormal in it; none: ``p = z``)::

    z^T S  p = (1 / pi) sum_k w_k Re[(C_k^-H z)^H Qf (C_k^-H Qq p)]      (eofs: adjoint solves only)
    z^T S' p = (1 / pi) sum_k w_k Re[(C_k^-1 z)^H Qq (C_k^-1 Qf p)]      (optimals: forward solves only)

and ``tr S = sum(theta) + E[z^T S p]`` over probes with ``E[z z^T] = I``; the ``n`` unit vectors give the sum itself."""

from __future__ import annotations

import numpy as np

import helpers  # noqa: F401
import stochastic_reference as ref  # noqa: F401

_GAMMA, _C1, _C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(x):
    """The output function of splitmix64 on ``uint64`` values (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + _GAMMA
        x = (x ^ (x >> np.uint64(30))) * _C1
        x = (x ^ (x >> np.uint64(27))) * _C2
        return x ^ (x >> np.uint64(31))


def probe_columns(n, indices, seed=0):
    """The Rademacher probes with the given probe indices as columns (``n x len(indices)``): entry ``(i, p)`` is ``+1`` where the top
    bit of ``mix(mix(mix(seed) + p) + i)`` is 0, else ``-1`` -- a pure function of ``(seed, p, i)``."""
    rows = np.arange(n, dtype=np.uint64)
    cols = []
    with np.errstate(over="ignore"):
        for p in indices:
            key = mix(mix(np.uint64(seed)) + np.uint64(p))
            cols.append(np.where(mix(key + rows) >> np.uint64(63), -1.0, 1.0))
    return np.column_stack(cols)


def probes(n, nprobes, seed=0):
    """Probes ``0 .. nprobes - 1`` of ``seed``: what ``lsa_stochastic_probes`` returns."""
    return probe_columns(n, range(nprobes), seed)


def deflated(host, Z, kind="eofs", U=None):
    """``P = Z - U (U^T Q Z)`` with ``Q`` the kind's weight (``U`` None: ``Z``)."""
    Z = np.asarray(Z, dtype=float)
    if U is None or U.shape[1] == 0:
        return Z
    return Z - U @ (U.T @ (host.weight(kind) @ Z))


def node_terms(host, Z, kind="eofs", U=None):
    """``N x R``: node ``k``'s share ``(w_k / pi) Re[y^H Q_mid x]`` of ``z_r^T S p_r``, by the two-column form: both columns through
    one direction's solves of the node."""
    Z = np.asarray(Z, dtype=float)
    Z = Z[:, None] if Z.ndim == 1 else Z
    P = deflated(host, Z, kind, U)
    out = np.zeros((len(host.nodes), Z.shape[1]))
    for k, h in enumerate(host.nodes):
        if kind == "eofs":
            Y, X, mid = h.solve_h(Z), h.solve_h(h.Qq @ P), h.Qf
        else:
            Y, X, mid = h.solve(Z), h.solve(h.Qf @ P), h.Qq
        out[k] = (host.weights[k] / np.pi) * np.einsum("ir,ir->r", Y.conj(), mid @ X).real
    return out


def forms(host, Z, kind="eofs", U=None):
    """``z_r^T S p_r`` for the columns of ``Z``: the node terms added in node order."""
    T = node_terms(host, Z, kind, U)
    out = np.zeros(T.shape[1])
    for k in range(T.shape[0]):
        out += T[k]
    return out


def one_column_terms(host, Z, kind="eofs", U=None):
    """The same node terms by the operator itself: ``z^T Re(W_k p) w_k / pi`` with ``HostStochastic.node_vectors`` (two dependent solves
    per node)."""
    Z = np.asarray(Z, dtype=float)
    P = deflated(host, Z, kind, U)
    c = host.weights / np.pi
    return np.column_stack([(Z[:, r] @ host.node_vectors(P[:, r], kind)) * c for r in range(Z.shape[1])])
