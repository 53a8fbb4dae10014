"""Grouping of eigenproblems for :func:`Solver.eigen.solve_batch` (pure Python: no device is touched here).

A parameter sweep (the eleven Reynolds numbers of ``.examples/eigenvalues.py:61-108``) solves problems ``(A_j, M_j, sigma_j)``
that share one sparsity pattern and one solver configuration.  Such problems can share one context, one fill-reducing
ordering, one pattern-only analysis of the exact LU and one set of index tables; only the numeric factorisation and the
iteration are per problem.  :func:`plan_batches` finds those groups; every other problem is solved alone.
"""

from __future__ import annotations

import hashlib
from dataclasses import dataclass, field

import numpy as np

from .utils import PreconditionerType, iEpsWhich, iSTType

MAX_BATCH = 16  # problems of one group (the batched sweeps take up to 16 factor sets: lsa_hip.NDLU_BATCH_MAX)


@dataclass
class BatchPlan:
    """``groups``: lists of solver indices that share one context, ordering and analysis, in input order; ``alone``: the
    indices solved one by one, with the reason for each."""

    groups: list[list[int]] = field(default_factory=list)
    alone: dict[int, str] = field(default_factory=dict)


def _pattern_digest(A, M) -> str:
    h = hashlib.sha1()
    for X in (A, M):
        if X is None:
            h.update(b"none")
            continue
        h.update(np.asarray(X.shape, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(X.indptr, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(X.indices, dtype=np.int64).tobytes())
    return h.hexdigest()


def batch_key(eps) -> tuple[tuple | None, str]:
    """``(key, "")`` for a solver that can join a group (solvers with equal keys can), ``(None, reason)`` otherwise.

    The key holds everything the solo path depends on apart from the values of ``(A, M)`` and the target: the sparsity
    patterns, the dimensions, tolerances and driver settings, whether the factors are real or complex, and -- on patterns
    dense enough for the library to eliminate zero-diagonal unknowns last -- the set of those unknowns."""
    if eps._A is None:
        return None, "operators are not set"
    if eps._which is iEpsWhich.ALL:
        return None, "spectrum slicing (iEpsWhich.ALL)"
    if eps._st_type is not iSTType.SINVERT:
        return None, f"spectral transformation {eps._st_type.name} (only SINVERT is batched)"
    if eps._pc_type not in (PreconditionerType.LU, PreconditionerType.CHOLESKY) or eps._ilu_levels is not None:
        return None, "not the exact LU"
    if eps._layout != "single":
        return None, "sharded layout"
    if eps._adjoint:
        return None, "adjoint problem"
    if getattr(eps, "_two_sided", False):
        return None, "two-sided solve"
    if eps._project_out is not None:
        return None, "projection (project_out)"
    if eps._ordering == "natural":
        return None, "natural ordering"
    A = eps._A.as_scipy_array()
    M = None if eps._M is None else eps._M.as_scipy_array()
    n = A.shape[0]
    if n <= 8:
        return None, "too small for the nested-dissection LU"
    sigma = complex(eps._target)
    cplx = A.dtype.kind == "c" or (M is not None and M.dtype.kind == "c") or sigma.imag != 0.0
    constraint = None
    if M is None or (A.nnz == M.nnz and np.array_equal(A.indptr, M.indptr) and np.array_equal(A.indices, M.indices)):
        if A.nnz > 60 * n:  # (Solver/utils.py prepare: the ordering eliminates zero-diagonal unknowns last on such patterns)
            K = A if M is None else A - sigma * M
            zd = np.asarray(K.diagonal() == 0)
            constraint = hashlib.sha1(np.packbits(zd).tobytes()).hexdigest() if zd.any() else None
    elif A.nnz + M.nnz > 60 * n:
        return None, "operators on different patterns with a dense union"
    key = (_pattern_digest(A, M), n, cplx, constraint, eps._problem_type, eps._nev, eps._ncv, eps._tol, eps._max_it, eps._which,
           eps._ksp_type, eps._ksp_rtol, eps._restart_len, eps._ksp_max_it, eps._ilu_shift, eps._ordering, eps._seed, eps._device,
           eps._lu, None if eps._antishift is None else complex(eps._antishift), bool(getattr(eps, "_symmetric", False)))
    return key, ""


def plan_batches(solvers, max_batch: int = 8, *, bytes_per_problem: int = 0, memory_budget: int = 0, keys=None) -> BatchPlan:
    """Groups of ``solvers`` (:class:`Solver.utils.iEpsSolver`) with equal :func:`batch_key`, in input order, at most
    ``max_batch`` per group -- and at most ``memory_budget // bytes_per_problem`` when both are given.  ``keys``: the results of
    :func:`batch_key` where the caller has them already (the frequencies of one resolvent sweep share one solver and one key)."""
    if not isinstance(max_batch, (int, np.integer)) or isinstance(max_batch, bool) or not 1 <= max_batch <= MAX_BATCH:
        raise ValueError(f"max_batch must be an integer in [1, {MAX_BATCH}], got {max_batch!r}")
    cap = int(max_batch)
    if bytes_per_problem > 0 and memory_budget > 0:
        cap = max(1, min(cap, int(memory_budget // bytes_per_problem)))
    plan = BatchPlan()
    open_groups: dict[tuple, list[int]] = {}
    for i, eps in enumerate(solvers):
        key, reason = batch_key(eps) if keys is None else keys[i]
        if key is None:
            plan.alone[i] = reason
            continue
        g = open_groups.get(key)
        if g is None or len(g) >= cap:
            g = []
            open_groups[key] = g
            plan.groups.append(g)
        g.append(i)
    return plan
