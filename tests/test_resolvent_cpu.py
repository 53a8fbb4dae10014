"""CPU suite of the resolvent analysis: the numpy restatement of the library's iteration (``tests/resolvent_reference.py``) pinned
against two dense routes to the optimal gains, the front end's argument errors, and the presence of the C-ABI entries.  The GPU
suite (``tests/test_gpu_resolvent.py``) holds the library to the bounds this restatement meets."""

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import resolvent_reference as ref


@pytest.mark.parametrize("omega", ref.OMEGAS)
def test_restatement_against_the_dense_routes(omega):
    """S2k (n = 1953), nev 4, ncv 12, tol 1e-10.  The two dense routes (singular values of M^(1/2) C^-1 M^(1/2); eigenvalues of W)
    give the listed six-decimal gains and agree to 1e-9 sigma_1 (the non-symmetric eigenvalue route is the less accurate one); the
    restatement matches the singular values to 1e-10 sigma_1 (the bound of the GPU suite), its projected matrix is real symmetric
    by construction with |Im h_j| at rounding level, it restarts, its pairs are M-orthonormal and R M f_j = sigma_j q_j."""
    A, M = ref.case("S2k")
    svd = ref.dense_gains_svd("S2k", omega)[:4]
    eig = ref.dense_gains_eig("S2k", omega)[:4]
    expected = np.array(ref.GAINS_S2K[omega])
    print(f"omega = {omega}: svd route {svd}, |svd - eig|_max / sigma_1 = {np.abs(svd - eig).max() / svd[0]:.2e}")
    assert np.allclose(svd, expected, rtol=0.0, atol=1e-5)
    assert np.allclose(eig, expected, rtol=0.0, atol=1e-5)
    assert np.abs(svd - eig).max() <= 1e-9 * svd[0]
    out = ref.resolvent_trl(A, M, omega, 4, 12, 1e-10, ref.start_vector(A.shape[0]))
    T = out["T"][:12, :12]
    oq, of, res = ref.pair_checks(A, M, omega, out["gains"], out["Q"], out["F"])
    print(f"restatement: {out['restarts']} restarts, {out['applies']} applies, |gain - svd|_max / sigma_1 = "
          f"{np.abs(out['gains'] - svd).max() / svd[0]:.2e}, max |Im h| / |alpha| = {out['imag_ratio']:.2e}, |Q^H M Q - I|_max = {oq:.2e}, "
          f"|F^H M F - I|_max = {of:.2e}, pair residual = {res:.2e}")
    assert len(out["gains"]) == 4 and np.allclose(out["gains"], expected, rtol=0.0, atol=1e-5)
    assert np.abs(out["gains"] - svd).max() <= 1e-10 * svd[0]
    assert T.dtype == np.float64 and np.array_equal(T, T.T)
    assert out["imag_ratio"] <= 1e-12
    assert out["restarts"] >= 1
    assert oq <= 1e-10 and of <= 1e-10 and res <= 1e-8
    for q in out["Q"].T:
        k = int(np.argmax(np.abs(q)))
        assert q[k].real > 0.0 and abs(q[k].imag) <= 1e-15 * abs(q[k])


def _pair():
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0.0], [0.0, 3.0, 1.0], [1.0, 0.0, 4.0]]))
    M = sp.identity(3, format="csr")
    return A, M


def test_front_end_argument_errors():
    """What the front end refuses before any device work (there is no device here)."""
    from Solver.resolvent import ResolventConfig, ResolventSolver
    from Solver.utils import PreconditionerType

    A, M = _pair()
    crooked = sp.csr_matrix(np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="symmetric"):
        ResolventSolver(A, crooked)
    with pytest.raises(ValueError, match="complex"):
        ResolventSolver(A, (M * (1.0 + 0.0j)).tocsr())
    with pytest.raises(ValueError, match="needs M"):
        ResolventSolver(A, None)
    with pytest.raises(ValueError, match="ncv"):
        ResolventSolver(A, M, ResolventConfig(num_modes=3, ncv=3))
    with pytest.raises(NotImplementedError, match="layout"):
        ResolventSolver(A, M, layout="sharded")
    with pytest.raises(NotImplementedError, match="exact LU"):
        ResolventSolver(A, M, pc_type=PreconditionerType.ILU)
    with pytest.raises(NotImplementedError, match="exact LU"):
        ResolventSolver(A, M, ilu_levels=2)
    rs = ResolventSolver(A, M, ResolventConfig(num_modes=1, ncv=2))
    with pytest.raises(ValueError, match="real"):
        rs.solve(0.4 + 0.1j)
    with pytest.raises(ValueError, match="real"):
        rs.sweep([0.4, 1j])
    with pytest.raises(ValueError, match="real"):
        rs.solve(float("nan"))
    assert rs.config.num_modes == 1 and ResolventConfig() == ResolventConfig(num_modes=3, ncv=24, atol=1e-8, max_it=500)


def test_library_and_binding_carry_the_entries():
    import lsa_hip

    lib = lsa_hip.load_library()
    for name in ("lsa_resolvent_create", "lsa_resolvent_destroy", "lsa_resolvent_set_row_permutation", "lsa_resolvent_set_start",
                 "lsa_resolvent_extend", "lsa_resolvent_basis", "lsa_resolvent_solve"):
        assert name in lsa_hip.SIGNATURES and hasattr(lib, name)
    assert hasattr(lsa_hip, "ResolventBasis")
