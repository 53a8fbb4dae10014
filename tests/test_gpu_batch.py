"""GPU tests of batches of same-pattern eigenproblems: the batched sweeps of the exact LU (``lsa_ndlu_solve_batch``) and
``Solver.eigen.solve_batch`` return, bit for bit, what each problem returns when solved alone."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# tabulated targets of the harness sweep (lsa-fw_amd/examples/eigenvalues.py), Re = 40, 45, ..., 90
REYNOLDS = tuple(range(40, 91, 5))
TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j), (0.03 + 0.742986662573986j),
           (0.05 + 0.744243299635422j), (0.061 + 0.7461282552275759j), (0.072 + 0.7461282552275759j), (0.085 + 0.744557458900781j),
           (0.09 + 0.742986662573986j), (0.1 + 0.7398450699203962j), (0.115 + 0.7351326809400116j))

_CASES = {}


def _case(name, re):
    from synthetic import fem

    if (name, re) not in _CASES:
        _CASES[(name, re)] = fem.cylinder_case(name, re=float(re))
    return _CASES[(name, re)]


def _solver(es, target, nev, atol, ncv=None, **kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    cfg = EigensolverConfig(num_eig=nev, atol=atol) if ncv is None else EigensolverConfig(num_eig=nev, atol=atol, ncv=ncv, max_it=500)
    s = EigenSolver(es.A, es.M, cfg, check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(target)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def _outcome(s):
    st = s.solver.stats
    return {"lam": s.solver._eigenvalues.copy(), "X": np.array(s.solver._eigenvectors), "restarts": st["krylov_restarts"],
            "applies": st["op_applies"], "shared": st.get("shared_analysis")}


def _solo(problems, **kw):
    out = []
    for es, target, nev, atol, ncv in problems:
        s = _solver(es, target, nev, atol, ncv, **kw)
        s.solve()
        out.append(_outcome(s))
        s.solver.release()
    return out


def _batched(problems, max_batch=8, **kw):
    from Solver.eigen import solve_batch

    solvers = [_solver(es, target, nev, atol, ncv, **kw) for es, target, nev, atol, ncv in problems]
    pairs = solve_batch(solvers, max_batch=max_batch)
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


# ---- the batched sweeps ----------------------------------------------------------------------------------------------------

def _factors(hip_ctx, name, res, targets):
    import lsa_hip

    out = []
    for re_, sigma in zip(res, targets):
        es = _case(name, re_)
        C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
        dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
        out.append((lsa_hip.NdLu(hip_ctx, dC, 0), dC))
    return out


@pytest.mark.parametrize("J,shifts,vdtype", [(1, "complex", np.complex128), (3, "complex", np.complex128), (3, "real", np.complex128),
                                             (3, "real", np.float64), (16, "complex_S2k", np.complex128)])
def test_ndlu_solve_batch_equals_solo_solves(hip_ctx, J, shifts, vdtype):
    """Complex factors (complex shifts), real factors with complex and with real vectors: each instance of the batched sweeps
    (the kernels at the batch's pointer capacity) against lsa_ndlu_solve per factor set (the same kernels at capacity one).
    J = 16 fills the pointer struct to its last slot: sixteen distinct complex shifts of one Reynolds number of S2k."""
    import lsa_hip

    name, res = ("S2k", REYNOLDS[:1] * J) if shifts == "complex_S2k" else ("S5k", REYNOLDS[:J])
    if shifts == "complex_S2k":
        targets = tuple(TARGETS[0] + 0.01 * j * (1 + 1j) for j in range(J))
    else:
        targets = TARGETS[:J] if shifts == "complex" else tuple(0.05 + 0.01 * j for j in range(J))
    assert len(set(targets)) == J == len(res)
    fs = _factors(hip_ctx, name, res, targets)
    n = fs[0][1].shape[0]
    rng = np.random.default_rng(11)
    bs = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(J)]
    if vdtype is np.float64:
        bs = [b.real.copy() for b in bs]
    solo = []
    for (f, _), b in zip(fs, bs):
        x = lsa_hip.DeviceVector(hip_ctx, n, vdtype)
        f.solve(lsa_hip.DeviceVector.from_numpy(hip_ctx, b), x)
        solo.append(x.numpy())
    dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
    dxs = [lsa_hip.DeviceVector(hip_ctx, n, vdtype) for _ in range(J)]
    lsa_hip.NdLu.solve_batch([f for f, _ in fs], dbs, dxs)
    for x, ref in zip(dxs, solo):
        assert np.array_equal(x.numpy(), ref)
    # in place (x = b) and repeated: the same bits again
    lsa_hip.NdLu.solve_batch([f for f, _ in fs], dbs, dbs)
    for x, ref in zip(dbs, solo):
        assert np.array_equal(x.numpy(), ref)


def test_ndlu_solve_batch_rejects_other_analyses(hip_ctx):
    import lsa_hip

    (f5, d5), = _factors(hip_ctx, "S5k", REYNOLDS[:1], TARGETS[:1])
    (f2, d2), = _factors(hip_ctx, "S2k", REYNOLDS[:1], TARGETS[:1])
    (fr, dr), = _factors(hip_ctx, "S5k", REYNOLDS[1:2], (0.05,))  # real shift: real factors
    n5, n2 = d5.shape[0], d2.shape[0]
    v5 = [lsa_hip.DeviceVector(hip_ctx, n5, np.complex128) for _ in range(4)]
    v2 = lsa_hip.DeviceVector(hip_ctx, n2, np.complex128)
    # (LSA_ERR_ARG reaches Python as ValueError)
    with pytest.raises(ValueError, match="same analysis"):
        lsa_hip.NdLu.solve_batch([f5, f2], [v5[0], v2], [v5[1], v2])
    with pytest.raises(ValueError, match="same analysis"):
        lsa_hip.NdLu.solve_batch([f5, fr], v5[:2], v5[2:])
    with pytest.raises(ValueError, match="share a factorisation"):
        lsa_hip.NdLu.solve_batch([f5, f5], v5[:2], v5[2:])
    with pytest.raises(ValueError, match="at most 16"):
        lsa_hip.NdLu.solve_batch([f5] * 17, v5[:1] * 17, v5[1:2] * 17)


# ---- solve_batch ------------------------------------------------------------------------------------------------------------

def _harness(name, idx):
    return [(_case(name, REYNOLDS[i]), TARGETS[i], 5, 1e-3, None) for i in idx]


def test_solve_batch_s5k_harness_configuration_equals_solo():
    problems = _harness("S5k", (0, 4, 9))
    _assert_same(_batched(problems), _solo(problems))


def test_solve_batch_of_one_equals_solo():
    problems = _harness("S5k", (2,))
    _assert_same(_batched(problems), _solo(problems))


def test_solve_batch_s30k_bench_configuration_restart_counts_differ():
    """Four Reynolds numbers of the bench case in its configuration (k = 20, ncv = 80, tol 1e-10): the problems take different
    numbers of restarts, and each still returns its solo bits."""
    idx = (0, 1, 5, 10)
    problems = [(_case("S30k", REYNOLDS[i]), TARGETS[i], 20, 1e-10, 80) for i in idx]
    batched, solo = _batched(problems, max_batch=4), _solo(problems)
    print("restarts:", [b["restarts"] for b in batched], "applies:", [b["applies"] for b in batched])
    assert len({b["restarts"] for b in batched}) > 1
    _assert_same(batched, solo)


def test_solve_batch_with_refinement_equals_solo(monkeypatch):
    """Spoilt factors (LSA_ND_TEST_PERTURB, as in test_gpu_3d.py): every inner solve takes the refinement step, in the batch
    as alone."""
    monkeypatch.setenv("LSA_ND_TEST_PERTURB", "1e-7")
    problems = _harness("S5k", (1, 6))
    _assert_same(_batched(problems), _solo(problems))


def test_solve_batch_followers_that_analyse_again_equal_solo(monkeypatch):
    """When a member's factorisation did not run on the group's analysis (stats["analysis_reused"] != 1: a zero pivot made the
    library analyse again), the next member runs the pattern-only phase again from the shared forest; here every member is
    told so, and each still returns its solo bits."""
    from Solver.utils import iEpsSolver

    calls = []
    real_redo = iEpsSolver.redo_pattern_phase
    monkeypatch.setattr(iEpsSolver, "stats", property(lambda self: {**self._stats, "analysis_reused": 0}))
    monkeypatch.setattr(iEpsSolver, "redo_pattern_phase", lambda self: (calls.append(1), real_redo(self)))
    problems = _harness("S5k", (0, 5, 8))
    batched = _batched(problems)
    assert len(calls) == 2
    monkeypatch.undo()
    _assert_same(batched, _solo(problems))


def test_solve_batch_projection_falls_back_to_solo():
    es = _case("S5k", REYNOLDS[3])
    keep_out = np.arange(0, es.A.shape[0], 3)[:50]
    problems = _harness("S5k", (3, 7))
    batched = _batched(problems, project_out=keep_out)
    _assert_same(batched, _solo(problems, project_out=keep_out), shared=False)


def test_harness_batch_writes_the_files_of_one_at_a_time(tmp_path):
    script = ROOT / "lsa-fw_amd" / "examples" / "eigenvalues.py"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "lsa-fw_amd")]))
    for mode, extra in (("one", ["--jobs", "1"]), ("batch", ["--batch", "4"])):
        cmd = [sys.executable, str(script), "--save-dir", str(tmp_path / mode), "--synthesize", "S5k", *extra]
        subprocess.run(cmd, check=True, env=env, cwd=str(tmp_path), timeout=900, capture_output=True)
    one = sorted((tmp_path / "one").rglob("sigma_eig0.txt"))
    assert len(one) == len(REYNOLDS)
    for f in one:
        g = tmp_path / "batch" / f.relative_to(tmp_path / "one")
        assert g.read_bytes() == f.read_bytes()
