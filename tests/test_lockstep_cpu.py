"""CPU suite of the lockstep Krylov-Schur driver: ``lsa_krylov_solve_batch`` and ``lsa_ks_batch_info`` are declared, exported and
bound with the layout the C side asserts; the planner caps a group by a device-memory budget without ever returning an empty
group; ``solve_batch`` refuses a ``lockstep`` that is not a bool before any device is touched."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import lsa_hip

HEADER = Path(__file__).resolve().parents[1] / "include" / "lsa_hip.h"


def _solver(j, n=40):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    A = sp.csr_matrix(sp.random(n, n, density=0.1, random_state=1, format="csr") + sp.eye(n, format="csr"))
    A.sort_indices()
    A.data = A.data * (1.0 + 0.1 * j)
    M = sp.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    es = EigenSolver(A, M, EigensolverConfig(num_eig=3, atol=1e-8), check_hermitian=False)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(0.3 + 0.1j)
    es.solver.set_st_pc_type(PreconditionerType.LU)
    return es


def test_lockstep_entry_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+lsa_krylov_solve_batch\s*\(", text)
    assert re.search(r"\}\s*lsa_ks_batch_info\s*;", text)
    lib = lsa_hip.load_library()
    assert hasattr(lib, "lsa_krylov_solve_batch")
    restype, argtypes = lsa_hip.SIGNATURES["lsa_krylov_solve_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert hasattr(lsa_hip.KrylovBasis, "solve_batch")


def test_batch_info_layout_matches_header():
    # three int64 counters, one double, two arrays of sixteen int64 (csrc/dense.hip static_asserts the same number)
    assert ctypes.sizeof(lsa_hip.lsa_ks_batch_info) == 3 * 8 + 8 + 2 * 16 * 8 == 288
    names = [name for name, _ in lsa_hip.lsa_ks_batch_info._fields_]
    assert names == ["rounds", "launches", "periods", "launches_per_round", "lockstep_steps", "solo_steps"]
    body = re.search(r"typedef struct \{([^}]*)\}\s*lsa_ks_batch_info\s*;", HEADER.read_text(), flags=re.S).group(1)
    declared = re.findall(r"\b(?:int64_t|double)\s+([a-z_]+)(?:\[16\])?\s*;", body)
    assert declared == names
    # one capacity: the batched sweeps, the batched DCGS2 records, the per-problem counters, the planner's largest group
    from Solver.batch import MAX_BATCH

    assert lsa_hip.NDLU_BATCH_MAX == MAX_BATCH == len(lsa_hip.lsa_ks_batch_info().lockstep_steps) == len(lsa_hip.lsa_ks_batch_info().solo_steps) == 16
    # the layouts the batch call shares with the solo one stay where tests/test_abi.py's neighbours pin them
    assert ctypes.sizeof(lsa_hip.lsa_ks_options) == 88 and ctypes.sizeof(lsa_hip.lsa_ks_result) == 56


def test_planner_memory_budget_caps_a_group_and_never_empties_it():
    from Solver.batch import plan_batches

    eps = [_solver(j).solver for j in range(7)]
    # room for three problems, for two and a half, for exactly one
    assert plan_batches(eps, max_batch=8, bytes_per_problem=1000, memory_budget=3000).groups == [[0, 1, 2], [3, 4, 5], [6]]
    assert plan_batches(eps, max_batch=8, bytes_per_problem=1000, memory_budget=2500).groups == [[0, 1], [2, 3], [4, 5], [6]]
    assert plan_batches(eps, max_batch=8, bytes_per_problem=1000, memory_budget=1000).groups == [[j] for j in range(7)]
    # a budget below one problem still plans every problem, one at a time (the solve then answers for the memory)
    plan = plan_batches(eps, max_batch=8, bytes_per_problem=1000, memory_budget=10)
    assert plan.groups == [[j] for j in range(7)] and all(plan.groups) and plan.alone == {}
    # max_batch stays the upper bound under a generous budget; no budget given: no cap
    assert plan_batches(eps, max_batch=4, bytes_per_problem=1, memory_budget=10**12).groups == [[0, 1, 2, 3], [4, 5, 6]]
    assert plan_batches(eps, max_batch=8, bytes_per_problem=1000).groups == [list(range(7))]


@pytest.mark.parametrize("bad", ["yes", 1, None])
def test_solve_batch_refuses_a_lockstep_that_is_no_bool(bad):
    from Solver.eigen import solve_batch

    with pytest.raises(TypeError, match="lockstep"):
        solve_batch([_solver(0), _solver(1)], lockstep=bad)
