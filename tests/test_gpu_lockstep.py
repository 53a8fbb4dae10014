"""GPU tests of the lockstep Krylov-Schur driver (``lsa_krylov_solve_batch``, ``Solver.eigen.solve_batch(lockstep=True)``): the
problems of a group advance one Arnoldi round at a time through batched sweeps and batched DCGS2 launches, and each returns,
bit for bit, what it returns when solved alone -- eigenvalues, eigenvectors, restarts and operator applies."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# tabulated targets of the harness sweep (lsa-fw_amd/examples/eigenvalues.py), Re = 40, 45, ..., 90
REYNOLDS = tuple(range(40, 91, 5))
TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j), (0.03 + 0.742986662573986j),
           (0.05 + 0.744243299635422j), (0.061 + 0.7461282552275759j), (0.072 + 0.7461282552275759j), (0.085 + 0.744557458900781j),
           (0.09 + 0.742986662573986j), (0.1 + 0.7398450699203962j), (0.115 + 0.7351326809400116j))

_CASES = {}
_SOLO = {}  # solo outcomes by problem and environment, computed once and shared by the tests


def _case(name, re):
    from synthetic import fem

    if (name, re) not in _CASES:
        _CASES[(name, re)] = fem.cylinder_case(name, re=float(re))
    return _CASES[(name, re)]


def _solver(problem, **kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    name, re, target, nev, atol, ncv = problem
    es = _case(name, re)
    cfg = EigensolverConfig(num_eig=nev, atol=atol) if ncv is None else EigensolverConfig(num_eig=nev, atol=atol, ncv=ncv, max_it=500)
    s = EigenSolver(es.A, es.M, cfg, check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(target)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def _outcome(s):
    st = s.solver.stats
    return {"lam": s.solver._eigenvalues.copy(), "X": np.array(s.solver._eigenvectors), "restarts": st["krylov_restarts"],
            "applies": st["op_applies"], "shared": st.get("shared_analysis"), "refined": st["refined_solves"],
            "lockstep": st.get("lockstep"), "lockstep_steps": st.get("lockstep_steps"), "solo_steps": st.get("solo_steps")}


def _solo(problems, env=(), **kw):
    out = []
    for p in problems:
        key = (p, tuple(env), tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in _SOLO:
            s = _solver(p, **kw)
            s.solve()
            _SOLO[key] = _outcome(s)
            s.solver.release()
        out.append(_SOLO[key])
    return out


def _lockstep(problems, max_batch=8, **kw):
    from Solver.eigen import solve_batch

    solvers = [_solver(p, **kw) for p in problems]
    pairs = solve_batch(solvers, max_batch=max_batch, lockstep=True)
    out = [_outcome(s) for s in solvers]
    for s, p in zip(solvers, pairs):  # what .solve() returns, and the solver stays usable
        assert [v for v, _ in p] == [s.solver.get_eigenvalue(i) for i in range(len(p))]
        assert np.all(np.isfinite(s.solver.residuals()))
    for s in solvers:
        s.solver.release()
    return out


def _assert_same(batched, solo, shared=True):
    assert len(batched) == len(solo)
    for b, s in zip(batched, solo):
        assert b["shared"] is shared
        assert np.array_equal(b["lam"], s["lam"])
        assert np.array_equal(b["X"], s["X"])
        assert b["restarts"] == s["restarts"] and b["applies"] == s["applies"]


def _harness(name, idx):
    return [(name, REYNOLDS[i], TARGETS[i], 5, 1e-3, None) for i in idx]


# ---- Solver.eigen.solve_batch(lockstep=True) -----------------------------------------------------------------------------------

def test_lockstep_s5k_harness_configuration_equals_solo():
    """The harness configuration: every member's steps run in lockstep rounds, and each returns its solo bits."""
    problems = _harness("S5k", (0, 4, 9))
    batched = _lockstep(problems)
    for b in batched:
        assert b["lockstep"] is True and b["lockstep_steps"] > 0
        assert b["lockstep_steps"] + b["solo_steps"] == b["applies"]
    _assert_same(batched, _solo(problems))


@pytest.mark.parametrize("J", [1, 16])
def test_lockstep_of_one_and_of_sixteen_equal_solo(J):
    """Sixteen distinct complex shifts of one Reynolds number of S2k fill the batched argument records to their last slot; a
    group of one runs the same driver with one problem per round."""
    problems = [("S2k", REYNOLDS[0], TARGETS[0] + 0.01 * j * (1 + 1j), 5, 1e-3, None) for j in range(J)]
    assert len({p[2] for p in problems}) == J
    batched = _lockstep(problems, max_batch=16)
    assert all(b["lockstep"] is True and b["lockstep_steps"] > 0 for b in batched)
    _assert_same(batched, _solo(problems))


def test_lockstep_s30k_bench_configuration_problems_at_different_steps():
    """Four Reynolds numbers of the bench case in its configuration (k = 20, ncv = 80, tol 1e-10): the problems keep different
    numbers of vectors at their restarts (so the rounds hold problems at different j) and leave after different numbers of
    restarts; each still returns its solo bits."""
    idx = (0, 1, 5, 10)
    problems = [("S30k", REYNOLDS[i], TARGETS[i], 20, 1e-10, 80) for i in idx]
    batched, solo = _lockstep(problems, max_batch=4), _solo(problems)
    print("restarts:", [b["restarts"] for b in batched], "applies:", [b["applies"] for b in batched],
          "lockstep steps:", [b["lockstep_steps"] for b in batched])
    assert len({b["restarts"] for b in batched}) > 1
    assert all(b["lockstep"] is True and b["lockstep_steps"] > 0 for b in batched)
    _assert_same(batched, solo)


def test_lockstep_all_members_spoilt_nobody_stays(monkeypatch):
    """Spoilt factors for the whole group (LSA_ND_TEST_PERTURB): every member's first check misses ksp_rtol, the refinement
    switch takes the tail form away and with it the lockstep set; all steps run through the solo code."""
    monkeypatch.setenv("LSA_ND_TEST_PERTURB", "1e-7")
    problems = _harness("S5k", (1, 6))
    batched = _lockstep(problems)
    for b in batched:
        assert b["lockstep"] is False and b["lockstep_steps"] == 0 and b["solo_steps"] == b["applies"] and b["refined"] > 0
    _assert_same(batched, _solo(problems, env=("perturb",)))


def test_lockstep_real_shifts_run_every_step_alone_and_equal_solo():
    """Real shifts on the real S5k pair: C = A - sigma M and its factors are real, and the tail form of a pipelined step takes
    a complex C only (``k_cgs2_tail_fits``, for the solo solve as well).  Such a group therefore never advances in lockstep:
    the library runs all steps of every member through the solo code inside the group's call (neither the batched sweeps nor
    the batched DCGS2 launches run on real factors), and each member returns its solo bits."""
    problems = [("S5k", REYNOLDS[j], 0.05 + 0.01 * j, 5, 1e-3, None) for j in range(3)]
    batched = _lockstep(problems)
    for b in batched:
        assert b["lockstep"] is False and b["lockstep_steps"] == 0 and b["solo_steps"] == b["applies"]
    _assert_same(batched, _solo(problems))


def test_lockstep_group_cut_into_chunks_by_the_memory_budget(monkeypatch):
    """A budget for two and a half problems cuts a group of five into chunks of 2, 2 and 1: every chunk is its own lockstep call
    on the group's context, every member after the first runs the pattern-only phase again, all equal their solo solves."""
    from Solver.utils import iEpsSolver

    calls = []
    real_redo = iEpsSolver.redo_pattern_phase
    monkeypatch.setattr(iEpsSolver, "lockstep_bytes_per_problem", lambda self: int(0.8 * self._prepared["ctx"].mem_info()[0] / 2.5))
    monkeypatch.setattr(iEpsSolver, "redo_pattern_phase", lambda self: (calls.append(1), real_redo(self)))
    problems = _harness("S5k", (0, 2, 4, 6, 9))
    batched = _lockstep(problems)
    monkeypatch.undo()
    assert len(calls) == 4
    assert all(b["lockstep"] is True and b["lockstep_steps"] > 0 for b in batched)
    _assert_same(batched, _solo(problems))


@pytest.mark.parametrize("batch", ["1", "16"])
def test_lockstep_does_not_depend_on_the_read_back_period(monkeypatch, batch):
    """LSA_KRYLOV_BATCH = 1 and = 16 under lockstep: the delayed form's basis must not depend on the steps per read-back, so both
    give the bits of the (default) solo solve."""
    problems = _harness("S5k", (0, 4, 9))
    solo = _solo(problems)
    monkeypatch.setenv("LSA_KRYLOV_BATCH", batch)
    batched = _lockstep(problems)
    assert all(b["lockstep"] is True for b in batched)
    _assert_same(batched, solo)


_DELAYED_OFF_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd", sys.argv[1] + "/tests"]
import numpy as np
import test_gpu_lockstep as t
problems = t._harness("S5k", (0, 4, 9))
batched, solo = t._lockstep(problems), t._solo(problems)
t._assert_same(batched, solo)
print(json.dumps({"lockstep": [b["lockstep"] for b in batched], "steps": [b["lockstep_steps"] for b in batched],
                  "solo_steps": [b["solo_steps"] for b in batched], "applies": [b["applies"] for b in batched]}))
"""


def test_lockstep_with_the_delayed_form_off_runs_every_member_alone():
    """LSA_KRYLOV_DELAYED=0 (read once per process: a child process): no member's steps take the DCGS2 tail form, so the library
    runs every member's steps through the solo code, one member after the other -- and each still equals its solo solve
    (asserted in the child)."""
    p = subprocess.run([sys.executable, "-c", _DELAYED_OFF_CHILD, str(ROOT)], env={**os.environ, "LSA_KRYLOV_DELAYED": "0"}, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["lockstep"] == [False] * 3 and rec["steps"] == [0] * 3 and rec["solo_steps"] == rec["applies"]


def test_lockstep_member_not_eligible_by_the_planner_runs_alone():
    es = _case("S5k", REYNOLDS[3])
    keep_out = np.arange(0, es.A.shape[0], 3)[:50]
    problems = _harness("S5k", (3, 7))
    batched = _lockstep(problems, project_out=keep_out)
    _assert_same(batched, _solo(problems, project_out=keep_out), shared=False)


# ---- lsa_hip.KrylovBasis.solve_batch --------------------------------------------------------------------------------------------

def _open_basis(ctx, re, sigma, ncv, spoil=False):
    import lsa_hip

    es = _case("S5k", re)
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, es.A), lsa_hip.CsrMatrix.from_scipy(ctx, es.M)
    if spoil:
        os.environ["LSA_ND_TEST_PERTURB"] = "1e-7"
    try:
        op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, sigma, pc_type=2, ksp_rtol=1e-8)
    finally:
        os.environ.pop("LSA_ND_TEST_PERTURB", None)
    return lsa_hip.KrylovBasis(ctx, op, ncv), op, (dA, dM)


def test_one_member_leaves_lockstep_the_others_stay(hip_ctx):
    """Three S5k operators, the middle one with spoilt factors: it takes the refinement switch at its first check and finishes
    through the solo code, the other two stay in lockstep; all three equal their solo solves (the middle one against a solo
    solve on the same spoilt factors)."""
    import lsa_hip

    idx, nev, ncv, tol = (0, 4, 9), 5, 25, 1e-3
    n = _case("S5k", REYNOLDS[0]).A.shape[0]
    rng = np.random.default_rng(0)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    solo = []
    for q, i in enumerate(idx):
        kb, op, keep = _open_basis(hip_ctx, REYNOLDS[i], TARGETS[i], ncv, spoil=q == 1)
        solo.append((kb.solve(nev, tol, 500, 7, 0, TARGETS[i], v0=v0), op.stats()))
        del kb, op, keep
    objs = [_open_basis(hip_ctx, REYNOLDS[i], TARGETS[i], ncv, spoil=q == 1) for q, i in enumerate(idx)]
    res, info = lsa_hip.KrylovBasis.solve_batch([o[0] for o in objs], nev, tol, 500, 7, 0, [TARGETS[i] for i in idx], v0s=v0)
    print("info:", info)
    stats = [o[1].stats() for o in objs]
    assert info["rounds"] > 0 and info["periods"] > 0 and info["launches_per_round"] > 3
    assert info["lockstep_steps"][1] == 0 and info["solo_steps"][1] > 0 and stats[1]["refined_solves"] > 0
    for z in (0, 2):
        assert info["lockstep_steps"][z] > 0 and info["solo_steps"][z] == 0 and stats[z]["refined_solves"] == 0
    for z in range(3):
        r, (s, sst) = res[z], solo[z]
        assert r.nconv >= nev
        assert np.array_equal(r.lam, s.lam) and np.array_equal(r.vectors, s.vectors) and np.array_equal(r.residuals, s.residuals)
        assert r.restarts == s.restarts and r.op_applies == s.op_applies
        assert info["lockstep_steps"][z] + info["solo_steps"][z] == r.op_applies
        for key in ("op_applies", "spmv_calls", "sptrsv_calls", "refined_solves"):
            assert stats[z][key] == sst[key], key


def test_argument_errors_reach_python_as_value_errors(hip_ctx):
    import lsa_hip
    from synthetic import fem

    a, opa, ka = _open_basis(hip_ctx, REYNOLDS[0], TARGETS[0], 25)
    b, opb, kb_ = _open_basis(hip_ctx, REYNOLDS[1], TARGETS[1], 25)
    c, opc, kc = _open_basis(hip_ctx, REYNOLDS[2], TARGETS[2], 20)  # another ncv
    call = lambda bases, **kw: lsa_hip.KrylovBasis.solve_batch(bases, 5, 1e-3, 500, 7, 0, [TARGETS[0]] * max(len(bases), 1), **kw)  # noqa: E731
    with pytest.raises(ValueError, match=r"J = 0 outside \[1, 16\]"):
        call([], ctx=hip_ctx)
    with pytest.raises(ValueError, match=r"J = 17 outside \[1, 16\]"):
        call([a] * 17)
    with pytest.raises(ValueError, match="share a workspace"):
        call([a, b, a])
    with pytest.raises(ValueError, match="another shape"):
        call([a, c])
    es2 = fem.cylinder_case("S2k")
    d2 = (lsa_hip.CsrMatrix.from_scipy(hip_ctx, es2.A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, es2.M))
    op2 = lsa_hip.ShiftInvertOperator(hip_ctx, d2[0], d2[1], TARGETS[0], pc_type=2)
    with pytest.raises(ValueError, match="another shape"):
        call([a, lsa_hip.KrylovBasis(hip_ctx, op2, 25)])
    other = lsa_hip.Context(0)
    try:
        o, opo, ko = _open_basis(other, REYNOLDS[1], TARGETS[1], 25)
        with pytest.raises(ValueError, match="another context"):
            call([a, o])
        del o, opo, ko
    finally:
        import gc

        gc.collect()
        other.close()
    # the refused calls left the workspaces usable
    res, info = lsa_hip.KrylovBasis.solve_batch([a, b], 5, 1e-3, 500, 7, 0, [TARGETS[0], TARGETS[1]])
    assert all(r.nconv >= 5 for r in res) and all(s > 0 for s in info["lockstep_steps"])
