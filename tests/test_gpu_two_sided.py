"""GPU suite of the two-sided eigensolve (``EigenSolver(..., two_sided=True)``): the direct phase returns the bits of the plain
solver, the left phase those of a fresh ``adjoint=True`` solver at the conjugated target, both on ONE factorisation; the pairing,
normalisation and condition numbers on top of them; ``lsa_eig_biorth`` against numpy; ``EigenSensitivitySolver.solve_pair``.

Every eigensolve is made once per module and shared (read only) by the tests that look at it."""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
_runs: dict = {}


def _solver(es, sigma, k, ncv, **kw):
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iSTType

    s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=k, atol=1e-10, ncv=ncv), check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(sigma)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def _trio(case: str, sigma, k: int = 6, ncv: int = 40, driver: str = "native"):
    """Plain, two-sided and fresh adjoint (at conj(sigma)) solves of one configuration, solved once; their results are read only."""
    import os

    from synthetic import fem

    key = (case, complex(sigma), k, ncv, driver)
    if key not in _runs:
        es = fem.cylinder_case(case)
        old = os.environ.get("LSA_KS_DRIVER")
        os.environ["LSA_KS_DRIVER"] = driver
        try:
            out = {"es": es}
            for name, target, kw in (("plain", sigma, {}), ("two", sigma, {"two_sided": True}), ("adjoint", np.conj(sigma), {"adjoint": True})):
                s = _solver(es, target, k, ncv, **kw)
                out[name + "_pairs"] = s.solve()
                out[name] = s.solver
                s.solver.release()  # (the results stay; the device copies go)
            _runs[key] = out
        finally:
            if old is None:
                del os.environ["LSA_KS_DRIVER"]
            else:
                os.environ["LSA_KS_DRIVER"] = old
    return _runs[key]


def _values_and_vectors(eps):
    n = eps.get_num_converged()
    return np.array([complex(eps.get_eigenvalue(i)) for i in range(n)]), np.column_stack([eps.get_eigenvector_array(i) for i in range(n)])


def _assert_phases_are_the_separate_solves(t):
    plain, two, adjoint = t["plain"], t["two"], t["adjoint"]
    lam_p, X_p = _values_and_vectors(plain)
    lam_t, X_t = _values_and_vectors(two)
    assert lam_p.shape == lam_t.shape and lam_p.tobytes() == lam_t.tobytes(), "right eigenvalues differ from the plain solver's"
    assert X_p.tobytes() == X_t.tobytes(), "right eigenvectors differ from the plain solver's"
    for (l0, v0), (l1, v1) in zip(t["plain_pairs"], t["two_pairs"]):  # what solve() hands out
        assert l0 == l1 and v0.real.as_array().tobytes() == v1.real.as_array().tobytes()
    mu_a, Z_a = _values_and_vectors(adjoint)
    mu_t, Z_t = two.get_adjoint_eigenpairs()
    assert mu_a.shape == mu_t.shape and mu_a.tobytes() == mu_t.tobytes(), "adjoint eigenvalues differ from the fresh adjoint solver's"
    assert np.ascontiguousarray(Z_a).tobytes() == np.ascontiguousarray(Z_t).tobytes(), "left vectors differ from the fresh adjoint solver's"
    # the direct phase's statistics are the plain solver's, in every counter
    st_p, st_t = plain.stats, two.stats
    left = st_t.pop("left")
    assert set(st_p) == set(st_t)
    for name in st_p:
        if not name.startswith("seconds"):
            assert st_p[name] == st_t[name], name
    # the left phase: its own figures, no factorisation, no analysis; its work is the fresh adjoint solver's
    assert left["refactored"] == 0 and left["seconds_factor"] == 0.0
    assert left["applies"] == adjoint.stats["op_applies"] > 0
    assert left["restarts"] == adjoint.stats["krylov_restarts"]
    assert left["converged"] == len(mu_a)
    for i in range(two.get_num_converged()):  # "unit": the adjoint iteration's vector as it is
        j = int(np.argmin(np.abs(np.conj(mu_a) - lam_t[i])))
        a = two.get_left_eigenvector_array(i, "unit")
        assert a is not None and a.tobytes() == Z_a[:, j].tobytes()


# ---- 5. bit equality, complex shift ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["native", "python"])
def test_phases_return_the_bits_of_the_separate_solves_complex_shift(driver):
    """S5k at SIGMA_RE50, k = 6, ncv = 40, atol 1e-10 (the configuration of ``test_adjoint_solver_matches_the_explicit_transposes``),
    through the library's outer loop and through its Python test double."""
    from synthetic import fem

    t = _trio("S5k", fem.SIGMA_RE50, driver=driver)
    assert t["two"].get_num_converged() >= 6
    _assert_phases_are_the_separate_solves(t)
    assert t["two"].stats["left"]["unmatched"] == 0


# ---- 6. bit equality, real shift --------------------------------------------------------------------------------------------------
def test_phases_return_the_bits_of_the_separate_solves_real_shift():
    """S5k at sigma = 0.05: real factors under complex vectors.  The spectrum of the real pencil is symmetric about the real axis:
    the eigenvalues come in conjugate pairs (or are real) and every pair finds its left partner."""
    t = _trio("S5k", 0.05)
    _assert_phases_are_the_separate_solves(t)
    two = t["two"]
    lam, _ = _values_and_vectors(two)
    print("real shift: eigenvalues", lam)
    for z in lam[:6]:
        assert np.min(np.abs(lam - np.conj(z))) <= 1e-8 * abs(z), f"{z} has no conjugate partner among {lam}"
    assert two.stats["left"]["unmatched"] == 0
    assert all(two.get_left_eigenvector_array(i) is not None for i in range(len(lam)))


# ---- 7. normalisation and defect -------------------------------------------------------------------------------------------------
def test_normalisation_left_residuals_and_off_diagonal_products():
    from synthetic import fem

    t = _trio("S5k", fem.SIGMA_RE50)
    es, two = t["es"], t["two"]
    A, M = es.A.tocsr(), es.M.tocsr()
    n = A.shape[0]
    lam, V = _values_and_vectors(two)
    k = len(lam)
    L = np.column_stack([two.get_left_eigenvector_array(i, "biorth") for i in range(k)])
    MV = M @ V
    G = L.conj().T @ MV
    print("biorth: max |a_i^H M v_i - 1| =", np.abs(np.diagonal(G) - 1.0).max(), " kappa =", two.get_condition_numbers(),
          " defect =", two.stats["left"]["biorth_defect"])
    assert np.abs(np.diagonal(G) - 1.0).max() <= 1e-10
    AH, MH = A.conj().T.tocsr(), M.conj().T.tocsr()
    R = A @ V - MV * lam[None, :]                 # right residual vectors r_j
    S = AH @ L - (MH @ L) * np.conj(lam)[None, :]  # left residual vectors s_i
    for i in range(k):
        assert np.linalg.norm(S[:, i]) <= 1e-8 * (np.linalg.norm(AH @ L[:, i]) + abs(lam[i]) * np.linalg.norm(MH @ L[:, i]))
    # (lam_i - lam_j) a_i^H M v_j = a_i^H r_j - s_i^H v_j
    na, nv, nmv = np.linalg.norm(L, axis=0), np.linalg.norm(V, axis=0), np.linalg.norm(MV, axis=0)
    nr, ns = np.linalg.norm(R, axis=0), np.linalg.norm(S, axis=0)
    worst = 0.0
    for i in range(k):
        for j in range(k):
            if i != j:
                bound = (na[i] * nr[j] + ns[i] * nv[j]) / abs(lam[i] - lam[j]) + 8 * n * EPS * na[i] * nmv[j]
                worst = max(worst, abs(G[i, j]) / bound)
                assert abs(G[i, j]) <= bound, (i, j, abs(G[i, j]), bound)
    print("off-diagonals: largest |a_i^H M v_j| / bound =", worst)
    # the defect of stats["left"] is the scaled off-diagonal maximum of the same matrix (device sums against host sums)
    d = np.abs(np.diagonal(G))
    off = np.abs(G) / np.sqrt(np.outer(d, d))
    np.fill_diagonal(off, 0.0)
    assert two.stats["left"]["biorth_defect"] == pytest.approx(off.max(), rel=1e-6, abs=8 * n * EPS * (na[:, None] * nmv[None, :]).max())
    # kappa by the formula, from the host products
    kappa = np.array([np.linalg.norm(two.get_left_eigenvector_array(i, "unit")) * nmv[i] for i in range(k)]) / np.array(
        [abs(np.vdot(two.get_left_eigenvector_array(i, "unit"), MV[:, i])) for i in range(k)])
    assert np.allclose(two.get_condition_numbers(), kappa, rtol=1e-9, atol=0)
    assert len(t["two_pairs"]) == 6


def test_left_eigenvectors_of_the_front_end_are_aligned_with_the_pairs():
    from synthetic import fem

    es = fem.cylinder_case("S2k")
    s = _solver(es, fem.SIGMA_RE50, 4, 40, two_sided=True)
    pairs = s.solve()
    lefts = s.left_eigenvectors()
    assert len(lefts) == len(pairs) == 4
    for (lam, v), a in zip(pairs, lefts):
        vv = v.real.as_array() + 1j * v.imag.as_array()
        aa = a.real.as_array() + 1j * a.imag.as_array()
        assert abs(np.vdot(aa, es.M @ vv) - 1.0) <= 1e-10
    unit = s.left_eigenvectors("unit")
    assert all(abs(np.linalg.norm(a.real.as_array() + 1j * a.imag.as_array()) - 1.0) <= 1e-12 for a in unit)
    with pytest.raises(ValueError):
        s.solver.get_left_eigenvector_array(0, "other")
    s.solver.release()


# ---- 8. condition numbers against the existing helper ------------------------------------------------------------------------
# Measured on MI355X (the two routes reach the same left eigenvectors through different shifts: the target here, every conj(lambda_i)
# in the helper): largest relative difference 5.9e-13 on S2k and 1.8e-10 on S5k; asserted is ten times the larger, rounded up
# to a power of ten.
KAPPA_AGREEMENT = 1e-8


@pytest.mark.parametrize("case", ["S2k", "S5k"])
def test_condition_numbers_agree_with_the_per_eigenvalue_helper(case):
    from helpers import eigenvalue_condition_numbers
    from synthetic import fem

    t = _trio(case, fem.SIGMA_RE50)
    two = t["two"]
    lam, V = _values_and_vectors(two)
    kappa = two.get_condition_numbers()[:6]
    ref = eigenvalue_condition_numbers(t["es"], lam[:6], V[:, :6])
    rel = np.abs(kappa - ref) / ref
    print(f"kappa {case}: two-sided {kappa}, helper {ref}, largest relative difference {rel.max():.3e}")
    assert np.isfinite(ref).all() and (kappa >= 1.0).all() and (ref >= 1.0).all()  # (ref: unclamped, from host products)
    assert rel.max() <= KAPPA_AGREEMENT


# ---- 9. lsa_eig_biorth against numpy -----------------------------------------------------------------------------------------------
def _check_biorth(hip_ctx, M, n, k, seed):
    import lsa_hip

    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
    Z = np.asfortranarray(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
    dM = None if M is None else lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    G, nz, nmx = lsa_hip.eig_biorth(hip_ctx, dM, X, Z)
    MX = X if M is None else M @ X
    ref = Z.conj().T @ MX
    rz, rmx = np.linalg.norm(Z, axis=0), np.linalg.norm(MX, axis=0)
    assert G.shape == (k, k)
    assert (np.abs(G - ref) <= 8 * n * EPS * np.outer(rz, rmx)).all(), np.abs(G - ref).max()
    assert (np.abs(nz - rz) <= 8 * n * EPS * rz).all() and (np.abs(nmx - rmx) <= 8 * n * EPS * rmx).all()
    G2, nz2, nmx2 = lsa_hip.eig_biorth(hip_ctx, dM, X, Z)
    assert G.tobytes() == G2.tobytes() and nz.tobytes() == nz2.tobytes() and nmx.tobytes() == nmx2.tobytes()
    return dM, X, nmx


@pytest.mark.parametrize("k", [1, 6, 20])
def test_biorth_entry_on_the_mass_matrix(hip_ctx, k):
    """The wrapper hands back host results only (G and the norms): the products M x_j never leave the device, so they cannot be
    compared with ``CsrMatrix.matvec`` bit for bit here.  They are ``k_spmv``'s, the function behind ``lsa_spmv``; what can be seen
    from outside is that ||M x_j|| is the fixed-order norm of exactly that product."""
    import lsa_hip
    from synthetic import fem

    M = fem.cylinder_case("S2k").M.tocsr()
    n = M.shape[0]
    dM, X, nmx = _check_biorth(hip_ctx, M, n, k, seed=k)
    x, y = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(X[:, 0])), lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
    dM.matvec(x, y)
    assert abs(nmx[0] - np.linalg.norm(y.numpy())) <= 8 * n * EPS * nmx[0]


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_biorth_entry_on_random_sparse_matrices(hip_ctx, n, kind):
    """Sub-wave and workgroup edges: one row, one short of a wavefront, one past a workgroup."""
    rng = np.random.default_rng(n)
    M = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format="csr") + sp.identity(n, format="csr")
    if kind == "complex":
        M = M + 1j * sp.random(n, n, density=min(1.0, 4.0 / n), random_state=rng, format="csr")
    M = sp.csr_matrix(M)
    M.sort_indices()
    _check_biorth(hip_ctx, M, n, 3, seed=7 * n)


def test_biorth_entry_without_a_matrix_and_its_refusals(hip_ctx):
    import lsa_hip

    _check_biorth(hip_ctx, None, 257, 5, seed=11)
    with pytest.raises(ValueError):
        lsa_hip.eig_biorth(hip_ctx, None, np.zeros((4, 2)), np.zeros((4, 3)))
    dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.identity(5, format="csr"))
    with pytest.raises(ValueError):  # LSA_ERR_ARG: M is 5 x 5, the vectors have 4 entries
        lsa_hip.eig_biorth(hip_ctx, dM, np.ones((4, 2)), np.ones((4, 2)))


# ---- 10. solve_pair ------------------------------------------------------------------------------------------------------------
def test_solve_pair_gives_direct_and_adjoint_mode_from_one_factorisation():
    from oracle import shift_invert
    from Sensitivity import EigenSensitivitySolver
    from synthetic import fem

    es = fem.cylinder_case("S2k")
    sigma = fem.SIGMA_RE50
    sens = EigenSensitivitySolver(es.A, es.M, target=sigma, tol_direct=1e-10, tol_adjoint=1e-10)
    lam, v, a = sens.solve_pair()
    ref, _, _ = shift_invert.solve(es.A, es.M, sigma, k=1, tol=1e-13)
    assert abs(lam - ref[0]) <= 1e-8 * abs(ref[0])
    assert abs(np.vdot(a, es.M @ v) - 1.0) <= 1e-10
    AHa = es.A.conj().T @ a
    assert np.linalg.norm(AHa - np.conj(lam) * (es.M.conj().T @ a)) <= 1e-7 * np.linalg.norm(AHa)
    ux, uy = es.node_offset, es.node_offset + 1
    sw = sens.compute_wavemaker(ux, uy)
    assert sw.shape == ux.shape and np.all(sw >= 0) and np.isfinite(sw).all() and sw.max() > 0
    left = sens.pair_stats["left"]
    assert left["refactored"] == 0 and left["seconds_factor"] == 0.0 and left["applies"] > 0
    assert sens.pair_stats["seconds_factor"] > 0.0  # the one factorisation, of the direct phase


# ---- 11. symmetric membrane -----------------------------------------------------------------------------------------------------
def test_symmetric_membrane_has_no_second_phase():
    from Solver.eigen import EigenSolver, EigensolverConfig
    from Solver.utils import PreconditionerType, iEpsProblemType, iSTType
    from synthetic import fem

    A, M, _ = fem.assemble_membrane(32, 32, 2.0, 4.0)
    es = EigenSolver(A, M, EigensolverConfig(num_eig=8, problem_type=iEpsProblemType.GHEP, atol=1e-10, ncv=32), symmetric=True, two_sided=True)
    es.solver.set_st_type(iSTType.SINVERT)
    es.solver.set_target(0.0)
    es.solver.set_st_pc_type(PreconditionerType.CHOLESKY)
    pairs = es.solve()
    s = es.solver
    assert s.stats["method"] == "lanczos" and len(pairs) == 8
    left = s.stats["left"]
    assert left["applies"] == 0 and left["restarts"] == 0 and left["unmatched"] == 0 and left["refactored"] == 0
    kappa = s.get_condition_numbers()
    print("membrane kappa", kappa)
    for i in range(s.get_num_converged()):
        assert s.get_left_eigenvector_array(i, "unit").tobytes() == s.get_eigenvector_array(i).tobytes()
    assert np.isfinite(kappa).all() and (kappa >= 1.0).all()
    # (the solver clamps rounding below 1 away, so the line above cannot see a kappa that is too small: the formula on the host can)
    V = np.column_stack([s.get_eigenvector_array(i) for i in range(s.get_num_converged())])
    MV = M @ V
    host = np.linalg.norm(V, axis=0) * np.linalg.norm(MV, axis=0) / np.abs(np.sum(V * MV, axis=0))
    n = A.shape[0]
    assert (host >= 1.0 - 4 * EPS).all() and (np.abs(kappa - host) <= 8 * n * EPS * host).all(), (kappa, host)
    lefts = es.left_eigenvectors()
    assert len(lefts) == 8 and all(a is not None and a.imag is None for a in lefts)
    s.release()
