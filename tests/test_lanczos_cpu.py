"""CPU suite: the host pieces of the symmetric path -- the dense symmetric eigen-solve ``lsa_dense_syev``, the decision function
``Solver.utils._symmetric_path`` and the numpy restatement of the thick-restart Lanczos iteration whose figures the GPU suite
(``tests/test_gpu_lanczos.py``) is held to."""

import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers  # noqa: F401

EPS = np.finfo(float).eps


def interior_membrane(nx, ny, a, b):
    """The interior pencil: ``assemble_membrane`` with the boundary dofs removed, symmetrised ``(X + X^T)/2``."""
    from synthetic import fem

    A, M, bnd = fem.assemble_membrane(nx, ny, a, b)
    keep = np.setdiff1d(np.arange(A.shape[0]), bnd)
    out = []
    for X in (A, M):
        Xi = sp.csr_matrix(X)[keep][:, keep]
        Xi = sp.csr_matrix((Xi + Xi.T) * 0.5)
        Xi.sort_indices()
        out.append(Xi)
    return out[0], out[1]


def on_shared_pattern(K, M):
    """Both matrices on the union of their sparsity patterns (explicit zeros), as the library's operator build wants them."""
    from Solver.utils import _onto_pattern

    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)  # noqa: E731
    union = (ones(K) + ones(M)).tocsr()
    union.sort_indices()
    return _onto_pattern(K, union), _onto_pattern(M, union)


# ---- 1. lsa_dense_syev ------------------------------------------------------------------------------------------------------------
def _syev_cases():
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 2, 3, 40, 200):
        d, e = rng.standard_normal(n), rng.standard_normal(max(n - 1, 0))
        cases.append((f"tridiagonal-{n}", np.diag(d) + np.diag(e, -1) + np.diag(e, 1)))
        B = rng.standard_normal((n, n))
        cases.append((f"dense-{n}", B + B.T))
    for n, k in ((40, 12), (200, 60)):  # after a thick restart: diagonal + spike + tridiagonal, couplings down to 1e-12
        T = np.zeros((n, n))
        T[np.arange(k), np.arange(k)] = rng.standard_normal(k)
        spike = 10.0 ** (-rng.uniform(0, 12, k))
        T[k, :k] = T[:k, k] = spike
        T[np.arange(k, n), np.arange(k, n)] = rng.standard_normal(n - k)
        off = 10.0 ** (-rng.uniform(0, 12, n - k - 1))
        T[np.arange(k + 1, n), np.arange(k, n - 1)] = off
        T[np.arange(k, n - 1), np.arange(k + 1, n)] = off
        cases.append((f"spike-{n}", T))
    B = rng.standard_normal((40, 40))
    cases.append(("entries-1e+90", (B + B.T) * 1e90))
    cases.append(("entries-1e-90", (B + B.T) * 1e-90))
    Q, _ = np.linalg.qr(rng.standard_normal((40, 40)))
    d = rng.standard_normal(40)
    d[:3] = 0.7
    A = (Q * d) @ Q.T
    cases.append(("threefold-40", (A + A.T) / 2))
    return cases


@pytest.mark.parametrize("name,A", _syev_cases(), ids=[c[0] for c in _syev_cases()])
def test_dense_syev_against_numpy_eigh(name, A):
    """Eigenvalues to 4 n eps ||A||_2, ||Q^T Q - I||_max <= 4 n eps, ||A Q - Q diag(w)||_max <= 8 n eps ||A||_2: loose multiples of
    the textbook O(n eps) of backward-stable tridiagonalisation + QL."""
    import lsa_hip

    n = A.shape[0]
    # only the lower triangle is read: garbage above the diagonal must not matter
    G = np.tril(A) + np.triu(np.full_like(A, 123.0), 1)
    w, Q = lsa_hip.dense_syev(G)
    ref = np.linalg.eigvalsh(A)
    norm2 = np.abs(ref).max()
    print(f"{name}: eig {np.abs(w - ref).max() / norm2:.2e}  orth {np.abs(Q.T @ Q - np.eye(n)).max():.2e}  "
          f"res {np.abs(A @ Q - Q * w).max() / norm2:.2e}  (n eps = {n * EPS:.2e})")
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - ref).max() <= 4 * n * EPS * norm2
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= 4 * n * EPS
    assert np.abs(A @ Q - Q * w).max() <= 8 * n * EPS * norm2


def test_dense_syev_rejects_bad_input():
    import lsa_hip

    with pytest.raises(lsa_hip.LsaError):
        lsa_hip.dense_syev(np.array([[1.0, 0.0], [np.nan, 1.0]]))
    w, Q = lsa_hip.dense_syev(np.zeros((0, 0)))
    assert w.shape == (0,)


# ---- 2. the decision function -----------------------------------------------------------------------------------------------------
def _membrane_solver(**kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType
    from synthetic import fem

    A, M, _ = fem.assemble_membrane(8, 8, 2.0, 4.0)
    ptype = kw.pop("problem_type", iEpsProblemType.GHEP)
    A = kw.pop("A", A)
    M = kw.pop("M", M)
    es = EigenSolver(A, M, EigensolverConfig(num_eig=4, problem_type=ptype, atol=1e-10, ncv=20), check_hermitian=False, symmetric=True, **kw)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(0.0)
    es.solver.set_st_pc_type(PreconditionerType.CHOLESKY)
    return es.solver


def test_symmetric_path_says_yes_for_the_membrane_pair():
    from Solver.utils import _symmetric_path, iEpsProblemType, symmetry_defect
    from synthetic import fem

    eps = _membrane_solver()
    assert _symmetric_path(eps) == (True, "")
    A, M, _ = fem.assemble_membrane(8, 8, 2.0, 4.0)
    assert symmetry_defect(A) <= 1e-12 and symmetry_defect(M) <= 1e-12
    eps.set_problem_type(iEpsProblemType.HEP)
    assert _symmetric_path(eps)[0]


def test_symmetric_path_says_no_with_a_reason_of_its_own():
    from Solver.utils import PreconditionerType, _symmetric_path, iEpsProblemType, iEpsWhich, iSTType
    from synthetic import fem

    reasons = {}

    def no(label, eps):
        ok, reason = _symmetric_path(eps)
        assert not ok and reason, label
        reasons[label] = reason

    no("gnhep", _membrane_solver(problem_type=iEpsProblemType.GNHEP))
    eps = _membrane_solver()
    eps.set_target(1.0 + 0.5j)
    no("complex target", eps)
    eps = _membrane_solver()
    eps.set_st_type(iSTType.SHIFT)
    no("shift", eps)
    no("ilu level", _membrane_solver(ilu_levels=1))
    no("adjoint", _membrane_solver(adjoint=True))
    A, M, _ = fem.assemble_membrane(8, 8, 2.0, 4.0)
    M = sp.csr_matrix(M).copy()
    r = M.shape[0] // 2
    c = M.indices[M.indptr[r]]  # an off-diagonal entry of an interior row
    assert c != r
    M[r, c] += 1e-6
    no("asymmetric M", _membrane_solver(M=M))
    eps = _membrane_solver()
    eps.set_which_eigenpairs(iEpsWhich.LARGEST_IMAGINARY)
    no("largest imaginary", eps)
    eps = _membrane_solver()
    eps.set_st_pc_type(PreconditionerType.ILU)
    no("ilu", eps)
    assert len(set(reasons.values())) == len(reasons), reasons
    assert "M is not symmetric" in reasons["asymmetric M"]


def test_symmetric_keyword_and_stats_keys_are_part_of_the_surface():
    from Solver.eigen import EigenSolver
    from Solver.utils import iEpsSolver

    for cls in (EigenSolver, iEpsSolver):
        p = inspect.signature(cls.__init__).parameters["symmetric"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    src = inspect.getsource(iEpsSolver.solve)
    for key in ('"method"', '"basis_bytes"', '"symmetric_fallback"'):
        assert key in src
    import lsa_hip

    for name in ("lsa_lanczos_create", "lsa_lanczos_destroy", "lsa_lanczos_set_row_permutation", "lsa_lanczos_set_start", "lsa_lanczos_extend",
                 "lsa_lanczos_basis", "lsa_lanczos_solve", "lsa_dense_syev"):
        assert name in lsa_hip.SIGNATURES and hasattr(lsa_hip.load_library(), name)
    assert hasattr(lsa_hip, "LanczosBasis") and hasattr(lsa_hip, "dense_syev")


def test_batch_groups_do_not_mix_symmetric_settings():
    from Solver.batch import batch_key
    from Solver.utils import iEpsSolver, PreconditionerType, iSTType

    A, M = interior_membrane(8, 8, 2.0, 2.0)
    keys = []
    for flag in (False, True):
        eps = iEpsSolver(A, M, symmetric=flag)
        eps.set_st_type(iSTType.SINVERT)
        eps.set_st_pc_type(PreconditionerType.LU)
        keys.append(batch_key(eps)[0])
    assert keys[0] is not None and keys[0] != keys[1]


# ---- 3. the numpy restatement of the iteration (what the GPU test is compared with) -------------------------------------------------
def lanczos_restatement(K, M, sigma, nev, ncv, tol, v0, max_restarts=50):
    """Thick-restart Lanczos for OP = (K - sigma M)^-1 M in the M-inner product, as lanczos.hip + lsa_lanczos_solve do it: full
    reorthogonalisation in two passes, T = diag + spike + tridiagonal, ranking by |lambda - sigma|, estimates |beta y_mi| / |theta_i|."""
    n, m = K.shape[0], ncv
    lu = spla.splu(sp.csc_matrix(K - sigma * M))
    V = np.zeros((n, m + 1))
    T = np.zeros((m + 1, m))
    t = M @ v0
    b = np.sqrt(v0 @ t)
    V[:, 0], rhs = v0 / b, t / b
    kept = restarts = applies = 0
    while True:
        for j in range(kept, m):
            w = lu.solve(rhs)
            applies += 1
            alpha = 0.0
            for _ in range(2):
                h = V[:, : j + 1].T @ (M @ w)
                w -= V[:, : j + 1] @ h
                alpha += h[j]
            t = M @ w
            beta = np.sqrt(w @ t)
            V[:, j + 1], rhs = w / beta, t / beta
            T[j, j], T[j + 1, j] = alpha, beta
            if j + 1 < m:
                T[j, j + 1] = beta
        theta, Y = np.linalg.eigh(T[:m, :m])
        beta = T[m, m - 1]
        lam = sigma + 1.0 / theta
        rank = np.argsort(np.abs(lam - sigma), kind="stable")
        rel = np.abs(beta * Y[m - 1, :]) / np.abs(theta)
        nconv = 0
        while nconv < m and rel[rank[nconv]] <= tol:
            nconv += 1
        if nconv >= nev or restarts >= max_restarts:
            sel = rank[:nconv]
            return lam[sel], V[:, :m] @ Y[:, sel], restarts, applies
        knew = max(min(nconv + (m - nconv) // 2, m - 1), 1)
        sel = rank[:knew]
        V[:, :knew] = V[:, :m] @ Y[:, sel]
        V[:, knew] = V[:, m]
        T[:] = 0.0
        T[np.arange(knew), np.arange(knew)] = theta[sel]
        T[knew, :knew] = T[:knew, knew] = beta * Y[m - 1, sel]
        kept = knew
        restarts += 1


def eig_residuals(K, M, lam, X):
    """The formula of ``lsa_eig_residuals``."""
    KX, MX = K @ X, M @ X
    return np.linalg.norm(KX - MX * lam, axis=0) / (np.linalg.norm(KX, axis=0) + np.abs(lam) * np.linalg.norm(MX, axis=0) + 1e-16)


@pytest.mark.parametrize("nx,ny,a,b,sigma,nev,ncv", [(32, 32, 2.0, 2.0, 10.0, 12, 40), (64, 64, 2.0, 4.0, 0.0, 24, 48)], ids=["32x32", "64x64-elasticity-shape"])
def test_restatement_meets_the_bounds_of_the_gpu_test(nx, ny, a, b, sigma, nev, ncv):
    K, M = interior_membrane(nx, ny, a, b)
    n = K.shape[0]
    lam, X, restarts, applies = lanczos_restatement(K, M, sigma, nev, ncv, 1e-10, np.random.default_rng(0).standard_normal(n))
    ref = spla.eigsh(K.tocsc(), k=nev, M=M.tocsc(), sigma=sigma, which="LM", tol=1e-13, return_eigenvectors=False)
    ref = ref[np.argsort(np.abs(ref - sigma), kind="stable")]
    assert len(lam) >= nev
    got = lam[:nev]
    err = np.abs(np.sort(got) - np.sort(ref)) / np.abs(np.sort(ref))
    G = X.T @ (M @ X)
    res = eig_residuals(K, M, lam, X)
    print(f"n = {n}: {restarts} restarts, {applies} applies, {len(lam)} pairs, eigenvalue error {err.max():.2e}, "
          f"|X^T M X - I| {np.abs(G - np.eye(len(lam))).max():.2e}, residual {res.max():.2e}")
    assert err.max() <= 1e-10
    assert np.abs(G - np.eye(len(lam))).max() <= 1e-10
    assert res.max() <= 1e-8
