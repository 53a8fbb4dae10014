"""CPU suite of the lockstep resolvent sweep: the chunk planner of ``ResolventSolver.sweep(lockstep=True)`` (order kept, real shifts
set aside, ``max_batch`` and budget cuts, results reassembled in input order, the library call behind a stub), the ``ValueError`` s of
the new keywords, and the presence of the new entry points in the header, the binding and the library.  The entries' argument errors
need handles, which need a device: ``tests/test_gpu_resolvent_lockstep.py::test_argument_errors_of_a_group`` holds them; what can be
reached with no context is checked here."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "lsa_hip.h"
NEW = ("lsa_spmv_batch", "lsa_resolvent_extend_batch", "lsa_resolvent_solve_batch")


def _solver(**kw):
    from Solver.resolvent import ResolventConfig, ResolventSolver

    n = 12
    A = sp.diags([np.arange(1.0, n + 1), np.ones(n - 1)], [0, 1], format="csr")
    M = sp.identity(n, format="csr")
    return ResolventSolver(A, M, ResolventConfig(num_modes=2, ncv=4), **kw)


def test_planner_keeps_order_and_sets_real_shifts_aside():
    rs = _solver()
    shifts = [0.5j, 0.0, 0.1 + 0.7j, 2.0, 0.9j, 1.1j, 1.3j]
    chunks, alone = rs.plan_lockstep(shifts, 8)
    assert chunks == [[0, 2, 4, 5, 6]] and alone == [1, 3]
    chunks, alone = rs.plan_lockstep(shifts, 2)
    assert chunks == [[0, 2], [4, 5], [6]] and alone == [1, 3]
    assert rs.plan_lockstep([1.0, 2.0], 8) == ([], [0, 1])
    assert rs.plan_lockstep([], 8) == ([], [])


def test_planner_cuts_at_sixteen_and_at_the_budget():
    rs = _solver()
    shifts = [1j * (0.1 + 0.05 * k) for k in range(35)]
    chunks, _ = rs.plan_lockstep(shifts, 40)
    assert [len(c) for c in chunks] == [16, 16, 3] and sum(chunks, []) == list(range(35))
    chunks, _ = rs.plan_lockstep(shifts[:5], 8, bytes_per_member=400, memory_budget=1000)
    assert [len(c) for c in chunks] == [2, 2, 1]
    chunks, _ = rs.plan_lockstep(shifts[:5], 8, bytes_per_member=4000, memory_budget=1000)  # (nothing fits: one at a time)
    assert [len(c) for c in chunks] == [1] * 5
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_batch"):
            rs.plan_lockstep(shifts, bad)


def test_sweep_reassembles_the_results_in_input_order(monkeypatch):
    """The library call behind a stub: every shift's result carries its own shift, the group call sees the chunks in order."""
    from Solver.resolvent import ResolventSolver

    calls = []

    def out_of(shift):
        return {"gains": np.array([abs(shift)]), "responses": np.zeros((12, 1), dtype=complex), "forcings": None, "estimates": np.zeros(1), "applies": 3}

    def group(self, shifts, nev, forcings):
        calls.append(("group", list(shifts)))
        return [(out_of(z), {"lockstep": True, "lockstep_steps": 3, "solo_steps": 0}) for z in shifts]

    def solo(self, shift, nev, forcings, warm=None):
        calls.append(("solo", shift))
        return out_of(shift), {}

    class Ctx:
        def mem_info(self):
            return (10**9, 10**9)

    monkeypatch.setattr(ResolventSolver, "_iterate_group", group)
    monkeypatch.setattr(ResolventSolver, "_iterate", solo)
    monkeypatch.setattr(ResolventSolver, "_prepare", lambda self, shift: ({}, Ctx(), None))
    monkeypatch.setattr(ResolventSolver, "_lockstep_bytes_per_member", lambda self, prep: 0)
    rs = _solver()
    omegas = [0.5, 0.0, 0.7, 0.9, 1.1]
    res = rs.sweep(omegas, lockstep=True, max_batch=3)
    assert [r.omega for r in res] == omegas and [float(r.gains[0]) for r in res] == omegas
    assert calls == [("group", [0.5j, 0.7j, 0.9j]), ("solo", 1.1j), ("solo", 0j)]
    assert [r.stats["lockstep"] for r in res] == [True, False, True, True, False]
    assert res[1].stats["solo_steps"] == 3 and res[1].stats["lockstep_steps"] == 0
    # the default path does not touch the planner
    calls.clear()
    assert [r.omega for r in rs.sweep(omegas)] == omegas and [c[0] for c in calls] == ["solo"] * 5
    # the map: points off the axis in groups, the real ones alone, the shape kept
    calls.clear()
    pts = np.array([[0.1 + 0.5j, 2.0], [0.2 + 0.6j, 0.3 + 0.7j]])
    gains = rs.norm_map(pts, warm_start=False, lockstep=True, max_batch=2)
    assert gains.shape == pts.shape and np.array_equal(gains, np.abs(pts))
    assert calls == [("group", [0.1 + 0.5j, 0.2 + 0.6j]), ("solo", 0.3 + 0.7j), ("solo", 2.0 + 0j)]


def test_value_errors_of_the_new_keywords():
    rs = _solver()
    with pytest.raises(ValueError, match="warm"):
        rs.norm_map([0.1 + 0.5j], warm_start=True, lockstep=True)
    with pytest.raises(ValueError, match="warm"):
        rs.norm_map([0.1 + 0.5j], lockstep=True)  # (warm_start defaults to on)
    with pytest.raises(ValueError, match="max_batch"):
        rs.sweep([0.4, 0.5], lockstep=True, max_batch=0)
    with pytest.raises(ValueError, match="real"):
        rs.sweep([0.4, 1j], lockstep=True)


def test_entries_are_declared_bound_and_exported():
    import lsa_hip

    text = HEADER.read_text()
    lib = lsa_hip.load_library()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", text), name
        assert name in lsa_hip.SIGNATURES and hasattr(lib, name), name
    for cls, name in ((lsa_hip.CsrMatrix, "spmv_batch"), (lsa_hip.ResolventBasis, "solve_batch"), (lsa_hip.ResolventBasis, "extend_batch")):
        assert callable(getattr(cls, name))
    declared = set(re.findall(r"^(?:int|void|const char \*|int64_t|double)\s*\*?\s*(lsa_[a-z0-9_]+)\(", text, flags=re.M))
    readme = (ROOT / "README.md").read_text()
    count = int(re.search(r"C-ABI \((\d+) entry points", readme).group(1))
    assert count == len(declared), (count, len(declared))


def test_argument_errors_reachable_without_a_context():
    """With no context there are no handles; the entries still refuse nulls with LSA_ERR_ARG instead of touching them."""
    import lsa_hip

    lib = lsa_hip.load_library()
    st = (ctypes.c_int32 * 1)()
    assert lib.lsa_spmv_batch(None, 1, None, None, None) == -1
    assert lib.lsa_resolvent_extend_batch(None, 1, None, None, None, 1, None, 2, None, st) == -1
    assert lib.lsa_resolvent_solve_batch(None, 1, None, None, None, 0, None, None, None, None, None, None, None, st, None) == -1
