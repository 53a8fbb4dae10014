"""GPU tests of ``Solver.utils.iKSP``: the linear solver that keeps its factorisation between solves."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

SIGMA = 0.018 + 0.7379601143282424j


def _shifted(case, sigma):
    from synthetic import fem

    es = fem.cylinder_case(case)
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    C.sort_indices()
    return C


def _direct(C):
    from Solver.utils import KSPType, PreconditionerType, iKSP

    ksp = iKSP(C)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(rtol=1e-12)
    return ksp


def _check(C, b, x, lu=None):
    res = np.linalg.norm(b - C @ x) / np.linalg.norm(b)
    assert res <= 1e-12, res
    if lu is not None:
        xref = lu.solve(b.astype(np.complex128))
        err = np.linalg.norm(x - xref) / np.linalg.norm(xref)
        print(f"|b - C x|/|b| = {res:.2e}, |x - x_SuperLU|/|x_SuperLU| = {err:.2e}")
        assert err <= 1e-10, err


def test_preonly_lu_keeps_its_factorisation():
    C = _shifted("S5k", SIGMA)
    n = C.shape[0]
    lu = spla.splu(C.tocsc().astype(np.complex128))
    rng = np.random.default_rng(3)
    b1 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    b2 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ksp = _direct(C)
    assert ksp.stats == {"analyses": 0, "factorisations": 0, "refactorisations": 0, "solves": 0, "columns": 0, "multi_width": 0}
    x1 = ksp.solve(b1).as_array()
    x2 = ksp.solve(b2).as_array()
    st = ksp.stats
    assert st["factorisations"] == 1 and st["analyses"] == 1 and st["refactorisations"] == 0 and st["solves"] == 2
    _check(C, b1, x1, lu)
    _check(C, b2, x2, lu)
    assert ksp.get_iteration_number() in (1, 2)
    assert ksp.get_residual_norm() <= 1e-12 * np.linalg.norm(b2)
    assert np.array_equal(ksp.get_solution().as_array(), x2)
    raw = ksp.raw
    assert raw.getType() == "preonly" and raw.getPC().getType() == "lu"
    assert raw.getIterationNumber() == ksp.get_iteration_number() and raw.getResidualNorm() == ksp.get_residual_norm()

    # the same pattern at a second shift: a refactorisation, no new analysis
    C2 = _shifted("S5k", SIGMA + 0.01j)
    ksp.set_operators(C2)
    x3 = ksp.solve(b1).as_array()
    st = ksp.stats
    assert st["refactorisations"] == 1 and st["analyses"] == 1 and st["factorisations"] == 1
    _check(C2, b1, x3, spla.splu(C2.tocsc().astype(np.complex128)))
    assert not np.array_equal(x3, x1)

    # several right-hand sides in one block solve: the bits of five solves
    B = rng.standard_normal((n, 5)) + 1j * rng.standard_normal((n, 5))
    solo = np.stack([ksp.solve(B[:, q]).as_array() for q in range(5)], axis=1)
    X = ksp.solve_many(B)
    assert X.shape == (n, 5) and np.array_equal(X, solo)
    assert ksp.stats["multi_width"] > 1
    assert ksp.stats["columns"] == 3 + 5 + 5
    # the adjoint system on the same factors
    XH = ksp.solve_many(B, adjoint=True)
    assert np.linalg.norm(B - C2.conj().T @ XH) <= 1e-12 * np.linalg.norm(B)
    assert ksp.stats["refactorisations"] == 1 and ksp.stats["factorisations"] == 1

    # another pattern: everything is rebuilt
    S2 = _shifted("S2k", SIGMA)
    ksp.set_operators(S2)
    bs = rng.standard_normal(S2.shape[0]) + 1j * rng.standard_normal(S2.shape[0])
    _check(S2, bs, ksp.solve(bs).as_array(), spla.splu(S2.tocsc().astype(np.complex128)))
    st = ksp.stats
    assert st["analyses"] == 2 and st["factorisations"] == 1 and st["refactorisations"] == 1

    # reset frees the device state; the next solve rebuilds it
    ksp.reset()
    assert ksp.stats["factorisations"] == 0
    xs = ksp.solve(bs).as_array()
    _check(S2, bs, xs)
    assert ksp.stats["factorisations"] == 1 and ksp.stats["analyses"] == 3
    with pytest.raises(ValueError):
        ksp.solve(bs[:-1])
    ksp.reset()


def test_gmres_without_preconditioner_and_a_nonzero_guess():
    """The small well-conditioned system of tests/test_gpu_linear.py's GMRES case: the velocity mass block of S2k."""
    from synthetic import fem
    from Solver.utils import KSPType, PreconditionerType, iKSP

    es = fem.cylinder_case("S2k")
    u = es.dofs_u[:300]  # velocity-velocity mass block: SPD (the pressure rows of M are zero)
    Mvv = es.M[u][:, u].tocsr()
    b = np.ones(300)
    rtol = 1e-10
    ksp = iKSP(Mvv)
    ksp.set_type(KSPType.GMRES)
    ksp.set_preconditioner(PreconditionerType.NONE)
    ksp.set_tolerances(rtol=rtol, max_it=300)
    x = ksp.solve(b).as_array()
    its = ksp.get_iteration_number()
    assert its > 0
    assert ksp.get_residual_norm() <= rtol * np.linalg.norm(b)
    assert np.linalg.norm(b - Mvv @ x) <= rtol * np.linalg.norm(b)
    assert ksp.raw.getType() == "gmres" and ksp.raw.getPC().getType() == "none"
    # the solution as the starting vector: fewer iterations than from zero
    from FEM.utils import iPETScVector

    ksp.set_initial_guess_nonzero(True)
    guess = iPETScVector(x)
    x2 = ksp.solve(b, guess)
    assert x2 is guess
    assert ksp.get_iteration_number() < its
    assert np.linalg.norm(b - Mvv @ x2.as_array()) <= rtol * np.linalg.norm(b)
    # columns one after another on this path; the adjoint needs the factors
    X = ksp.solve_many(np.stack([b, 2.0 * b], axis=1))
    assert np.linalg.norm(np.stack([b, 2.0 * b], axis=1) - Mvv @ X) <= rtol * np.linalg.norm(b) * np.sqrt(5)
    with pytest.raises(NotImplementedError):
        ksp.solve_many(np.stack([b, b], axis=1), adjoint=True)
    ksp.reset()


def test_solve_many_refines_the_one_column_that_missed(monkeypatch):
    """One column of a block spoilt before its check (its solution scaled by 1 + 1e-6 in place): that column alone takes the
    refinement step -- a block solve of one column on the block's vectors -- and the others keep their bits."""
    from Solver.utils import iKSP

    C = _shifted("S2k", SIGMA)
    n = C.shape[0]
    rng = np.random.default_rng(8)
    B = rng.standard_normal((n, 5)) + 1j * rng.standard_normal((n, 5))
    ksp = _direct(C)
    clean = ksp.solve_many(B)
    assert ksp.get_iteration_number() == 1
    calls = []
    true_residual = iKSP._residual

    def spoil_third(self, dev, bp, xp, adjoint=False):
        calls.append(len(calls))
        if len(calls) == 3:
            xp *= 1.0 + 1e-6
        return true_residual(self, dev, bp, xp, adjoint)

    monkeypatch.setattr(iKSP, "_residual", spoil_third)
    X = ksp.solve_many(B)
    assert len(calls) == 5 + 1  # every column, then the check of the one that missed after its step
    assert ksp.get_iteration_number() == 2
    for q in (0, 1, 3, 4):
        assert np.array_equal(X[:, q], clean[:, q])
    assert np.linalg.norm(B[:, 2] - C @ X[:, 2]) <= 1e-12 * np.linalg.norm(B[:, 2])
    assert np.linalg.norm(X[:, 2] - clean[:, 2]) <= 1e-10 * np.linalg.norm(clean[:, 2])
    ksp.reset()
