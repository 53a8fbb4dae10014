"""GPU suite: symmetric-definite eigenproblems on the real thick-restart Lanczos path (``lanczos.hip``, ``lsa_lanczos_solve``,
``EigenSolver(..., symmetric=True)``) against scipy's ``eigsh`` on the interior membrane pencils, whose square case carries nearly
double eigenvalues.  The bounds are those the numpy restatement in ``tests/test_lanczos_cpu.py`` is held to."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401
from test_lanczos_cpu import interior_membrane, on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent

# (nx, ny, a, b, sigma, nev, ncv): the three inputs of the suite
INPUTS = {
    "32x32": (32, 32, 2.0, 2.0, 10.0, 12, 40),
    "128x128": (128, 128, 2.0, 2.0, 10.0, 12, 40),
    "64x64-elasticity-shape": (64, 64, 2.0, 4.0, 0.0, 24, 48),
}


def symmetric_solver(K, M, sigma, nev, ncv, symmetric, problem_type=None):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType

    cfg = EigensolverConfig(num_eig=nev, problem_type=problem_type or iEpsProblemType.GHEP, atol=1e-10, ncv=ncv)
    es = EigenSolver(K, M, cfg, check_hermitian=False, symmetric=symmetric)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(sigma)
    es.solver.set_st_pc_type(PreconditionerType.CHOLESKY)
    return es


def eigsh_nearest(K, M, sigma, k):
    ref = spla.eigsh(sp.csc_matrix(K), k=k, M=sp.csc_matrix(M), sigma=sigma, which="LM", tol=1e-13, return_eigenvectors=False)
    return ref[np.argsort(np.abs(ref - sigma), kind="stable")]


def run_child(job, out, **env):
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, str(HERE / "lanczos_child.py"), job, str(out)], check=True, env=e, timeout=600)
    return np.load(out)


def lanczos_checks(K, M, Tfull, V, m):
    """(|V^T M V - I|_max, ||OP V_m - V_m T - beta v_{m+1} e_m^T||_F, ||T||_F), OP applied by scipy's splu."""
    T = Tfull[:m, :m]
    G = V.T @ (M @ V)
    lu = spla.splu(sp.csc_matrix(K - 10.0 * M))
    R = lu.solve(M @ V[:, :m]) - V[:, :m] @ T
    R[:, m - 1] -= Tfull[m, m - 1] * V[:, m]
    return np.abs(G - np.eye(m + 1)).max(), np.linalg.norm(R), np.linalg.norm(T)


def test_basis_and_lanczos_relation(hip_ctx, tmp_path):
    """40 steps through lsa_lanczos_extend: ||V^T M V - I||_max <= 1e-12 (two passes of classical Gram-Schmidt leave O(eps) times
    cond(M)^(1/2) < 1e2) and ||OP V_m - V_m T - beta v_{m+1} e_m^T||_F <= 1e-10 ||T||_F (the inner solves' ksp_rtol of 1e-12 times
    ||OP||), OP applied by scipy's splu.  A fresh process gives the same bits."""
    import lsa_hip

    K, M = interior_membrane(32, 32, 2.0, 2.0)
    n, m = K.shape[0], 40
    Ku, Mu = on_shared_pattern(K, M)
    dK, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, Ku), lsa_hip.CsrMatrix.from_scipy(hip_ctx, Mu)
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dK, dM, 10.0, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.LanczosBasis(hip_ctx, op, m)
    basis.set_start(np.random.default_rng(0).standard_normal(n))
    Tfull = np.zeros((m + 1, m), order="F")
    assert basis.extend(0, m, Tfull) == -1
    V = basis.basis(m + 1)
    del basis, op
    T = Tfull[:m, :m]
    assert np.array_equal(T, T.T) and np.count_nonzero(np.triu(T, 2)) == 0
    orth, defect, tn = lanczos_checks(K, M, Tfull, V, m)
    print(f"|V^T M V - I|_max = {orth:.2e}; relation defect / |T|_F = {defect / tn:.2e}")
    assert orth <= 1e-12
    assert defect <= 1e-10 * tn
    fused = run_child("basis", tmp_path / "fused.npz")
    assert np.array_equal(fused["T"], Tfull) and np.array_equal(fused["V"], V)


def test_fused_kernels_against_the_unfused_form(tmp_path):
    """The same 40 steps with LSA_LANCZOS_FUSED=0 (k_multi_dot + k_multi_axpy) in a child process: the unfused basis meets the
    bounds of the test above, and T and V of the two forms agree to 1e-12 ||T||_F.

    A Krylov basis amplifies rounding differences: the numpy restatement of tests/test_lanczos_cpu.py run twice on the CPU, the
    dots summed forwards and backwards, differs by |dT|_max = 1.6e-10 and |dV|_max = 6.7e-09 after these 40 steps, and a first
    version of the fused kernels with a summation order of its own differed from the unfused form by 1.6e-09 and 8.0e-08.  The
    fused kernels therefore add in the order of k_multi_dot and k_multi_axpy: on an MI355X the two forms give the same bits
    (|dT|_max = |dV|_max = 0), which is why this test cannot tell by the numbers that the knob reached the other form."""
    K, M = interior_membrane(32, 32, 2.0, 2.0)
    m = 40
    fused = run_child("basis", tmp_path / "fused.npz")
    plain = run_child("basis", tmp_path / "plain.npz", LSA_LANCZOS_FUSED="0")
    assert int(plain["bd"]) == -1
    orth, defect, tn = lanczos_checks(K, M, plain["T"], plain["V"], m)
    print(f"unfused: |V^T M V - I|_max = {orth:.2e}; relation defect / |T|_F = {defect / tn:.2e}")
    assert orth <= 1e-12
    assert defect <= 1e-10 * tn
    dT, dV = np.abs(plain["T"] - fused["T"]).max(), np.abs(plain["V"] - fused["V"]).max()
    print(f"fused against unfused: |dT|_max = {dT:.2e}, |dV|_max = {dV:.2e}, 1e-12 |T|_F = {1e-12 * tn:.2e}")
    assert dT <= 1e-12 * tn and dV <= 1e-12 * tn


_SOLVED = {}


def solved(name, symmetric):
    """One solve per (input, setting) and process: (solver, eigenvalues, vectors, eigsh reference, K, M)."""
    key = (name, symmetric)
    if key not in _SOLVED:
        nx, ny, a, b, sigma, nev, ncv = INPUTS[name]
        K, M = interior_membrane(nx, ny, a, b)
        es = symmetric_solver(K, M, sigma, nev, ncv, symmetric)
        es.solve()
        s = es.solver
        k = s.get_num_converged()
        lam = [s.get_eigenvalue(i) for i in range(k)]
        X = np.column_stack([s.get_eigenvector_array(i) for i in range(k)])
        _SOLVED[key] = (s, lam, X, eigsh_nearest(K, M, sigma, nev + 4), K, M)
    return _SOLVED[key]


@pytest.mark.parametrize("name", list(INPUTS))
def test_eigenpairs_on_the_symmetric_path(name):
    """Every one of the nev eigenvalues nearest sigma, at its rank, to 1e-10 relative; X^T M X = I to 1e-10; residuals <= 1e-8; real
    results.  On the square inputs both members of each nearly double pair are there, with M-orthogonal vectors."""
    nx, ny, a, b, sigma, nev, ncv = INPUTS[name]
    s, lam, X, ref, K, M = solved(name, True)
    assert s.stats["method"] == "lanczos" and "symmetric_fallback" not in s.stats
    assert len(lam) >= nev and all(type(v) is float for v in lam)
    v0 = s.get_eigenvector(0)
    assert X.dtype == np.float64 and not v0.is_complex and abs(v0.as_array().real @ (M @ v0.as_array().real) - 1.0) <= 1e-10
    got = np.array(lam[:nev])
    err = np.abs(got - ref[:nev]) / np.abs(ref[:nev])
    G = X.T @ (M @ X)
    res = s.residuals()
    print(f"{name}: {len(lam)} pairs, {s.stats['krylov_restarts']} restarts, {s.stats['op_applies']} applies; eigenvalue error {err.max():.2e}, "
          f"|X^T M X - I| {np.abs(G - np.eye(len(lam))).max():.2e}, residual {res.max():.2e}")
    assert err.max() <= 1e-10
    assert np.abs(G - np.eye(len(lam))).max() <= 1e-10
    assert res.max() <= 1e-8
    for c in range(X.shape[1]):  # deterministic sign: the entry of largest magnitude is positive
        assert X[np.argmax(np.abs(X[:, c])), c] > 0
    if name == "128x128":
        srt = np.sort(got)
        close = [(i, i + 1) for i in range(nev - 1) if abs(srt[i + 1] - srt[i]) <= 1e-6 * abs(srt[i])]
        refs = np.sort(ref[:nev])
        assert close == [(i, i + 1) for i in range(nev - 1) if abs(refs[i + 1] - refs[i]) <= 1e-6 * abs(refs[i])] and len(close) >= 3
        order = np.argsort(got)
        for i, j in close:
            assert abs(G[order[i], order[j]]) <= 1e-10


@pytest.mark.parametrize("name", ["32x32", "64x64-elasticity-shape"])
def test_general_path_agrees_and_holds_twice_the_basis(name):
    """symmetric=False on the same inputs: the eigenvalues of the symmetric run to 1e-8 relative (the general path projects an
    operator that is self-adjoint only in the M-norm orthogonally in the 2-norm: first order in its 1e-10 tolerance times
    cond(M)^(1/2) < 1e2); its basis arrays are twice as large."""
    nev = INPUTS[name][5]
    s1, lam1, _, _, _, _ = solved(name, True)
    s0, lam0, _, _, _, _ = solved(name, False)
    assert s0.stats["method"] == "arnoldi" and "symmetric_fallback" not in s0.stats
    d = np.abs(np.array(lam0[:nev]) - np.array(lam1[:nev])) / np.abs(np.array(lam1[:nev]))
    print(f"{name}: general against symmetric eigenvalues {d.max():.2e}; basis bytes {s0.stats['basis_bytes']} / {s1.stats['basis_bytes']}")
    assert d.max() <= 1e-8
    assert 0 < 2 * s1.stats["basis_bytes"] <= s0.stats["basis_bytes"]


def test_two_fresh_processes_give_identical_bytes(tmp_path):
    r1 = run_child("solve", tmp_path / "a.npz")
    r2 = run_child("solve", tmp_path / "b.npz")
    assert r1["lam"].shape[0] >= 12
    assert r1["lam"].tobytes() == r2["lam"].tobytes() and r1["X"].tobytes() == r2["X"].tobytes()


def test_fallbacks_run_and_say_so():
    """GNHEP with symmetric=True is today's solve, bit for bit, and says why; an indefinite M falls back with the reason the library
    gave and still finds the eigenvalues."""
    from synthetic import fem
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType

    es = fem.cylinder_case("S2k")
    out = []
    for flag in (False, True):
        solver = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=4, atol=1e-10, ncv=40), check_hermitian=False, symmetric=flag)
        solver.solver.set_st_type(iSTType.SINVERT)
        solver.solver.set_target(fem.SIGMA_RE50)
        solver.solver.set_st_pc_type(PreconditionerType.LU)
        solver.solve()
        s = solver.solver
        k = s.get_num_converged()
        out.append((np.array([s.get_eigenvalue(i) for i in range(k)]), np.column_stack([s.get_eigenvector_array(i) for i in range(k)]), s.stats))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert "symmetric_fallback" not in out[0][2] and "GNHEP" in out[1][2]["symmetric_fallback"]
    assert out[0][2]["method"] == out[1][2]["method"] == "arnoldi"

    K, M = interior_membrane(32, 32, 2.0, 2.0)
    neg = symmetric_solver(K, sp.csr_matrix(-M), -10.0, 12, 40, True, problem_type=iEpsProblemType.GHEP)
    neg.solve()
    s = neg.solver
    assert s.stats["method"] == "arnoldi" and "positive definite" in s.stats["symmetric_fallback"]
    got = np.array([s.get_eigenvalue(i) for i in range(12)])
    ref = -eigsh_nearest(K, M, 10.0, 12)
    print(f"indefinite M: {s.stats['symmetric_fallback']}; eigenvalue error {np.abs((got - ref) / ref).max():.2e}")
    assert np.abs((got - ref) / ref).max() <= 1e-8


def test_interval_sweep_on_the_symmetric_path():
    """iEpsWhich.ALL on [4, 33]: the eight eigenvalues eigsh finds there, to 1e-8 as the existing interval test asks, complete by count."""
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import iEpsProblemType, iEpsWhich

    K, M = interior_membrane(32, 32, 2.0, 2.0)
    want = np.array([4.93480665, 12.33704701, 12.33708130, 19.73949194, 24.67441242, 24.67441243, 32.07697510, 32.07772017])
    es = EigenSolver(K, M, EigensolverConfig(problem_type=iEpsProblemType.GHEP, num_eig=4, atol=1e-10), check_hermitian=False, symmetric=True)
    es.solver.set_interval(4.0, 33.0)
    es.solver.set_which_eigenpairs(iEpsWhich.ALL)
    es.solver.solve()
    s = es.solver
    got = np.array([s.get_eigenvalue(i) for i in range(s.get_num_converged())])
    print("interval:", got, s.stats.get("method"), s.stats.get("interval_expected"), s.stats.get("interval_complete"))
    assert s.stats["method"] == "lanczos"
    assert len(got) == 8 and np.allclose(got, want, rtol=0, atol=1e-8)
    assert s.stats["interval_expected"] == 8 and s.stats["interval_complete"] == 1


def test_elasticity_shaped_call_on_the_full_membrane_pair():
    """The reference's Elasticity call (GHEP, target 0, SINVERT, CHOLESKY, 24 modes) on the full 64 x 64, a = 2, b = 4 pair: the
    256-fold lambda = 1 of the Dirichlet rows is dropped as the reference's benchmark drops it; the first five other values."""
    from synthetic import fem
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType

    A, M, _ = fem.assemble_membrane(64, 64, 2.0, 4.0)
    es = EigenSolver(A, M, EigensolverConfig(num_eig=24, problem_type=iEpsProblemType.GHEP, atol=1e-10), symmetric=True)
    es.solver.set_target(0.0)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_st_pc_type(PreconditionerType.CHOLESKY)
    es.solver.set_dimensions(24, 48)
    es.solve()
    s = es.solver
    assert s.stats["method"] == "lanczos"
    lam = np.array([s.get_eigenvalue(i) for i in range(s.get_num_converged())])
    rest = lam[np.abs(lam - 1.0) > 1e-8]
    print(f"{len(lam)} pairs, {len(lam) - len(rest)} copies of lambda = 1; the others: {rest[:6]}")
    # eigsh on the same pair, shifted to 8 so that the copies of lambda = 1 stay out of its reach: its six nearest values are the first
    # six non-spurious ones (3.08, 4.93, 8.02, 10.49 and the pair at 12.337)
    ref = np.sort(spla.eigsh(sp.csc_matrix(A), k=6, M=sp.csc_matrix(M), sigma=8.0, which="LM", tol=1e-13, return_eigenvectors=False))[:5]
    assert np.allclose(ref, [3.08425155, 4.93480376, 8.01906231, 10.48645771, 12.33701662], rtol=0, atol=1e-8)
    assert len(rest) >= 5
    print(f"against eigsh: {np.max(np.abs(rest[:5] - ref) / ref):.2e}")
    assert np.max(np.abs(rest[:5] - ref) / ref) <= 1e-10
    ana = fem.membrane_analytic(5)
    assert np.max(np.abs(rest[:5] - ana) / ana) <= 2e-4


def test_standard_problem_on_the_symmetric_path():
    """HEP (no M: the inner product is the 2-norm, the products with M are skipped): eigenvalues against numpy's eigvalsh to 1e-10
    relative, orthonormal real vectors, residuals <= 1e-8."""
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType

    n = 400
    rng = np.random.default_rng(3)
    d, e = np.arange(1.0, n + 1.0), 0.3 * rng.standard_normal(n - 1)
    A = sp.diags([e, d, e], [-1, 0, 1], format="csr")
    exact = np.linalg.eigvalsh(A.toarray())
    sigma, nev = 100.4, 8
    es = EigenSolver(A, None, EigensolverConfig(num_eig=nev, problem_type=iEpsProblemType.HEP, atol=1e-10, ncv=24), symmetric=True)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(sigma)
    es.solver.set_st_pc_type(PreconditionerType.LU)
    es.solve()
    s = es.solver
    assert s.stats["method"] == "lanczos"
    got = np.array([s.get_eigenvalue(i) for i in range(nev)])
    want = exact[np.argsort(np.abs(exact - sigma), kind="stable")][:nev]
    X = np.column_stack([s.get_eigenvector_array(i) for i in range(nev)])
    print(f"HEP: eigenvalue error {np.abs((got - want) / want).max():.2e}, |X^T X - I| {np.abs(X.T @ X - np.eye(nev)).max():.2e}, "
          f"residual {s.residuals().max():.2e}")
    assert np.abs((got - want) / want).max() <= 1e-10
    assert X.dtype == np.float64 and np.abs(X.T @ X - np.eye(nev)).max() <= 1e-10
    assert s.residuals().max() <= 1e-8
