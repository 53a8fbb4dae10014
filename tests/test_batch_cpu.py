"""CPU suite: the batch entry points are declared, exported and bound; the planner behind ``Solver.eigen.solve_batch``
groups same-pattern, same-configuration problems and sends everything else to solo solves; bad input fails before any
device is touched."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import lsa_hip

HEADER = Path(__file__).resolve().parents[1] / "include" / "lsa_hip.h"


def _pair(n=40, seed=0, re_=1.0, shift_pattern=False):
    rng = np.random.default_rng(seed)
    A = sp.csr_matrix(sp.random(n, n, density=0.1, random_state=2 if shift_pattern else 1, format="csr") + sp.eye(n, format="csr"))
    A.sort_indices()
    A.data = A.data * re_ + rng.standard_normal(A.nnz) * 1e-3
    M = sp.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return A, M


def _solver(A, M, target, *, pc=None, st=None, nev=3, **kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    es = EigenSolver(A, M, EigensolverConfig(num_eig=nev, atol=1e-8), check_hermitian=False, **kw)
    es.solver.set_st_type(st or iSTType.SINVERT)
    es.solver.set_target(target)
    es.solver.set_st_pc_type(pc or PreconditionerType.LU)
    return es


def test_batch_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\blsa_ndlu_solve_batch\s*\(", text)
    lib = lsa_hip.load_library()
    assert hasattr(lib, "lsa_ndlu_solve_batch")
    restype, argtypes = lsa_hip.SIGNATURES["lsa_ndlu_solve_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 5
    assert lsa_hip.NDLU_BATCH_MAX == 16
    from Solver import solve_batch
    from Solver.eigen import solve_batch as sb

    assert solve_batch is sb


def test_planner_groups_same_pattern_and_configuration():
    from Solver.batch import plan_batches

    solvers = [_solver(*_pair(re_=1.0 + 0.1 * j), 0.3 + 0.01j * (j + 1)) for j in range(5)]
    plan = plan_batches([s.solver for s in solvers], max_batch=8)
    assert plan.groups == [[0, 1, 2, 3, 4]] and plan.alone == {}


def test_planner_splits_groups_at_max_batch_and_memory():
    from Solver.batch import plan_batches

    solvers = [_solver(*_pair(re_=1.0 + 0.1 * j), 0.3 + 0.1j) for j in range(7)]
    eps = [s.solver for s in solvers]
    assert plan_batches(eps, max_batch=3).groups == [[0, 1, 2], [3, 4, 5], [6]]
    assert plan_batches(eps, max_batch=1).groups == [[j] for j in range(7)]
    # a device-memory budget for two problems caps the groups below max_batch
    assert plan_batches(eps, max_batch=8, bytes_per_problem=100, memory_budget=250).groups == [[0, 1], [2, 3], [4, 5], [6]]


def test_planner_separates_patterns_and_factor_types():
    from Solver.batch import plan_batches

    a = _solver(*_pair(), 0.3 + 0.1j)
    b = _solver(*_pair(shift_pattern=True), 0.3 + 0.1j)  # another pattern
    c = _solver(*_pair(), 0.3)  # real shift: real factors
    d = _solver(*_pair(re_=2.0), 0.2 + 0.2j)
    e = _solver(*_pair(), 0.3 + 0.1j, nev=4)  # another configuration
    plan = plan_batches([x.solver for x in (a, b, c, d, e)])
    assert plan.groups == [[0, 3], [1], [2], [4]] and plan.alone == {}


def test_planner_sends_unsupported_settings_alone():
    from Solver.batch import plan_batches
    from Solver.utils import PreconditionerType, iEpsWhich, iSTType

    A, M = _pair()
    ok = _solver(A, M, 0.3 + 0.1j)
    shift = _solver(A, M, 0.3 + 0.1j, st=iSTType.SHIFT)
    cayley = _solver(A, M, 0.3 + 0.1j, st=iSTType.CAYLEY)
    ilu = _solver(A, M, 0.3 + 0.1j, pc=PreconditionerType.ILU)
    proj = _solver(A, M, 0.3 + 0.1j, project_out=np.array([0, 1]))
    adj = _solver(A, M, 0.3 + 0.1j, adjoint=True)
    sharded = _solver(A, M, 0.3 + 0.1j, layout="sharded")
    interval = _solver(A, M, 0.3 + 0.1j)
    interval.solver.set_which_eigenpairs(iEpsWhich.ALL)
    plan = plan_batches([x.solver for x in (ok, shift, cayley, ilu, proj, adj, sharded, interval)])
    assert plan.groups == [[0]]
    assert sorted(plan.alone) == [1, 2, 3, 4, 5, 6, 7]
    assert "SHIFT" in plan.alone[1] and "CAYLEY" in plan.alone[2] and "LU" in plan.alone[3]
    assert "project" in plan.alone[4] and "adjoint" in plan.alone[5] and "sharded" in plan.alone[6] and "ALL" in plan.alone[7]


def test_planner_splits_on_different_zero_diagonal_constraints():
    """On patterns dense enough for the ordering to eliminate zero-diagonal unknowns last, problems whose zero diagonals differ
    get different orderings: they cannot share one."""
    from Solver.batch import plan_batches

    n = 130
    dense = sp.csr_matrix(np.ones((n, n)))
    dense.sort_indices()
    A1 = dense.copy()
    A2 = dense.copy()
    M = sp.csr_matrix((np.zeros(dense.nnz), dense.indices.copy(), dense.indptr.copy()), shape=dense.shape)
    A1.setdiag(0.0)  # explicit zeros on the diagonal (structure kept)
    A2.data[:] = 1.0
    s1, s2, s3 = _solver(A1, M, 0.3 + 0.1j), _solver(A2, M, 0.3 + 0.1j), _solver(A1.copy(), M, 0.2 + 0.1j)
    plan = plan_batches([s.solver for s in (s1, s2, s3)])
    assert plan.groups == [[0, 2], [1]]


@pytest.mark.parametrize("bad", [0, 17, -1, 2.5, True, "4"])
def test_bad_max_batch_raises_before_any_device(bad):
    from Solver.eigen import solve_batch

    s = _solver(*_pair(), 0.3 + 0.1j)
    with pytest.raises(ValueError, match="max_batch"):
        solve_batch([s], max_batch=bad)
    assert s.solver._prepared is None  # nothing was prepared: no context was opened


def test_bad_solver_lists_raise_before_any_device():
    from Solver.eigen import solve_batch

    s = _solver(*_pair(), 0.3 + 0.1j)
    with pytest.raises(ValueError):
        solve_batch([])
    with pytest.raises(ValueError, match="more than once"):
        solve_batch([s, s])
    with pytest.raises(TypeError):
        solve_batch([s, s.solver])
    assert s.solver._prepared is None


def test_ndlu_solve_batch_checks_its_arguments_on_the_host():
    class Fake:
        def __init__(self, ctx):
            self.ctx, self.handle = ctx, ctypes.c_void_p(1)

    with pytest.raises(ValueError):
        lsa_hip.NdLu.solve_batch([], [], [])
    ctx = object()
    f = [Fake(ctx) for _ in range(17)]
    with pytest.raises(ValueError, match="at most 16"):
        lsa_hip.NdLu.solve_batch(f, f, f)
    with pytest.raises(ValueError, match="as many"):
        lsa_hip.NdLu.solve_batch(f[:2], f[:1], f[:2])
    with pytest.raises(ValueError, match="one context"):
        lsa_hip.NdLu.solve_batch([f[0], Fake(object())], f[:2], f[:2])


def test_shared_context_closes_with_its_last_user():
    from Solver.utils import SharedContext

    s = SharedContext()
    s.users += 2
    assert not s.drop() and not s.drop() and s.drop()
