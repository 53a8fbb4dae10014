"""CPU suite of the two-sided eigensolve: what runs without a device -- the pairing of direct and adjoint eigenvalues, the map of
``which`` under conjugation, the figures taken from the Gram matrix, the refusals raised before any device work, the batch planner."""

import numpy as np
import pytest
import scipy.sparse as sp

from Solver.batch import plan_batches
from Solver.eigen import EigenSolver, EigensolverConfig
from Solver.utils import (PreconditionerType, _conj_target, _lambda_rank_key, biorth_figures, conjugate_which, iEpsProblemType, iEpsSolver, iEpsWhich, iSTType,
                          pair_left_right)

SUPPORTED = ("LARGEST_MAGNITUDE", "LARGEST_REAL", "SMALLEST_REAL", "LARGEST_IMAGINARY", "SMALLEST_IMAGINARY", "TARGET_MAGNITUDE", "TARGET_REAL",
             "TARGET_IMAGINARY")


# ---- 1. pairing ---------------------------------------------------------------------------------------------------------------------
def test_pairing_exact_conjugates_in_shuffled_order():
    rng = np.random.default_rng(0)
    lam = rng.standard_normal(9) + 1j * rng.standard_normal(9)
    order = rng.permutation(9)
    match = pair_left_right(lam, np.conj(lam)[order])
    assert np.array_equal(order[match], np.arange(9))  # mu[match[i]] = conj(lam[i])


def test_pairing_with_a_missing_left_member_leaves_one_unmatched():
    lam = np.array([1.0 + 1j, 2.0 - 1j, 3.0 + 0.5j, -1.0 + 2j])
    mu = np.conj(lam[[3, 0, 2]])  # no partner for lam[1]
    match = pair_left_right(lam, mu)
    assert list(match) == [1, -1, 2, 0] and int((match < 0).sum()) == 1


def test_pairing_keeps_only_the_mutual_pair_when_two_share_a_nearest_neighbour():
    lam = np.array([1.0 + 0j, 1.1 + 0j])
    mu = np.array([1.08 + 0j, 5.0 + 0j])  # both direct values are nearest to mu[0]; mu[0] is nearest to lam[1]
    assert list(pair_left_right(lam, mu)) == [-1, 0]


def test_pairing_of_empty_inputs():
    assert pair_left_right(np.zeros(0), np.zeros(0)).shape == (0,)
    assert list(pair_left_right(np.array([1.0, 2.0]), np.zeros(0))) == [-1, -1]
    assert pair_left_right(np.zeros(0), np.array([1.0])).shape == (0,)


def test_pairing_involves_no_tolerance():
    """Eigenvalues that disagree in the first digit are still paired when they are each other's nearest."""
    lam = np.array([1.0 + 1j, 100.0 + 0j])
    mu = np.conj(np.array([130.0 + 5j, 1.4 + 0.7j]))
    assert list(pair_left_right(lam, mu)) == [1, 0]


# ---- 2. which under conjugation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SUPPORTED)
def test_conjugated_key_orders_the_conjugated_set_as_the_key_orders_the_set(name):
    rng = np.random.default_rng(3)
    lam = rng.standard_normal(40) + 1j * rng.standard_normal(40)
    target = 0.3 - 0.8j
    which = iEpsWhich[name]
    mapped = conjugate_which(which)
    direct = np.argsort(_lambda_rank_key(which, target)(lam), kind="stable")
    adjoint = np.argsort(_lambda_rank_key(mapped, np.conj(target))(np.conj(lam)), kind="stable")
    assert np.array_equal(direct, adjoint)
    swapped = {"LARGEST_IMAGINARY": "SMALLEST_IMAGINARY", "SMALLEST_IMAGINARY": "LARGEST_IMAGINARY"}
    assert mapped.name == swapped.get(name, name)
    assert conjugate_which(mapped) is which


def test_conjugated_real_target_keeps_its_positive_zero():
    """A solver set up at conj(0.05) stores 0.05 + 0j; the left phase must back-transform with the same number, zero signs included."""
    z = _conj_target(0.05)
    assert z == 0.05 and np.copysign(1.0, z.imag) == 1.0
    assert _conj_target(0.018 + 0.7j) == 0.018 - 0.7j
    assert np.copysign(1.0, _conj_target(np.complex128(2.0)).imag) == 1.0


# ---- the figures from the Gram matrix ---------------------------------------------------------------------------------------------
def test_figures_from_a_gram_matrix():
    G = np.array([[2.0 + 0j, 0.1j, 0.0], [0.2, 0.5j, 0.0], [0.0, 0.0, 0.0]])
    kappa, degenerate, defect = biorth_figures(G, np.array([1.0, 1.0, 1.0]), np.array([4.0, 3.0, 2.0]))
    assert kappa[0] == 2.0 and kappa[1] == 6.0 and np.isinf(kappa[2])
    assert list(degenerate) == [False, False, True]
    assert defect == pytest.approx(0.2 / np.sqrt(2.0 * 0.5))  # the degenerate pair is left out
    kappa, degenerate, defect = biorth_figures(np.zeros((0, 0)), np.zeros(0), np.zeros(0))
    assert kappa.shape == (0,) and defect == 0.0
    kappa, degenerate, _ = biorth_figures(np.array([[1e-320 + 0j]]), np.ones(1), np.ones(1))  # 1 / |d| overflows
    assert np.isinf(kappa[0]) and degenerate[0]


# ---- 3. validation, before any device work ----------------------------------------------------------------------------------------
def _pair(n=12):
    A = sp.diags([np.arange(1.0, n + 1), np.full(n - 1, 0.3)], [0, 1], format="csr")
    return A, sp.identity(n, format="csr")


def _solver(**kw):
    A, M = _pair()
    s = EigenSolver(A, M, EigensolverConfig(num_eig=2, atol=1e-8, ncv=8), check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(0.5)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def test_two_sided_with_adjoint_is_a_value_error():
    A, M = _pair()
    with pytest.raises(ValueError, match="two_sided"):
        EigenSolver(A, M, check_hermitian=False, adjoint=True, two_sided=True)
    eps = iEpsSolver(A, M, adjoint=True)
    with pytest.raises(ValueError, match="two_sided"):
        eps.set_two_sided(True)
    assert eps.get_two_sided() is False


def test_setter_and_getter():
    s = _solver()
    assert s.solver.get_two_sided() is False
    s.solver.set_two_sided(True)
    assert s.solver.get_two_sided() is True
    assert _solver(two_sided=True).solver.get_two_sided() is True
    with pytest.raises(RuntimeError, match="two_sided"):
        _solver().solver.get_condition_numbers()  # no two-sided solve has run


def _refused(configure, **kw):
    s = _solver(two_sided=True, **kw)
    configure(s.solver)
    s.solver._open = lambda: pytest.fail("the refusal must come before the operator is opened")
    s.solver.prepare = lambda *a, **k: pytest.fail("the refusal must come before anything is prepared")
    with pytest.raises(NotImplementedError, match="two_sided=True needs shift-invert"):
        s.solver.solve()


def test_shift_is_refused():
    _refused(lambda eps: eps.set_st_type(iSTType.SHIFT))


def test_cayley_is_refused():
    _refused(lambda eps: eps.set_st_type(iSTType.CAYLEY))


def test_ilu_is_refused():
    _refused(lambda eps: eps.set_st_pc_type(PreconditionerType.ILU))
    _refused(lambda eps: None, ilu_levels=2)


def test_sharded_layout_is_refused():
    _refused(lambda eps: None, layout="sharded")


def test_projection_is_refused():
    _refused(lambda eps: None, project_out=np.array([0, 1]))


def test_spectrum_slicing_is_refused():
    A, M = _pair()
    s = EigenSolver(A, M, EigensolverConfig(num_eig=2, problem_type=iEpsProblemType.GHEP), check_hermitian=False, two_sided=True)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    s.solver.set_interval(0.0, 3.0)
    s.solver.set_which_eigenpairs(iEpsWhich.ALL)
    with pytest.raises(NotImplementedError, match="iEpsWhich.ALL"):
        s.solver.solve()


# ---- 4. planner and ABI ----------------------------------------------------------------------------------------------------------
def test_planner_solves_a_two_sided_solver_alone_and_still_groups_the_others():
    from synthetic import fem

    es = fem.cylinder_case("S2k")

    def make(**kw):
        s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=2, atol=1e-8, ncv=20), check_hermitian=False, **kw)
        s.solver.set_st_type(iSTType.SINVERT)
        s.solver.set_target(fem.SIGMA_RE50)
        s.solver.set_st_pc_type(PreconditionerType.LU)
        return s.solver

    plan = plan_batches([make(), make(two_sided=True), make(), make(adjoint=True)], 8)
    assert plan.groups == [[0, 2]]
    assert plan.alone == {1: "two-sided solve", 3: "adjoint problem"}


def test_the_new_entry_is_declared_bound_and_exported():
    """(the agreement of header, binding and library as a whole is ``tests/test_abi.py``'s)"""
    import lsa_hip
    from test_abi import declared_functions

    assert "lsa_eig_biorth" in declared_functions() and "lsa_eig_biorth" in lsa_hip.SIGNATURES
    assert hasattr(lsa_hip.load_library(), "lsa_eig_biorth")
    assert len(lsa_hip.SIGNATURES["lsa_eig_biorth"][1]) == 9
