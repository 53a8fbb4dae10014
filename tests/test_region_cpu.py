"""CPU suite of the region eigensolver: the numpy / SuperLU restatement (``tests/region_reference.py``) pinned against the dense
spectrum of the S2k pencil, the node and weight formulas, the ``Rectangle`` geometry and every refusal of the front end (none of
which touches a device)."""

import numpy as np
import pytest

import region_reference as rr
from Solver.region import Ellipse, Rectangle, RegionConfig, RegionEigenSolver, contour_nodes


@pytest.mark.parametrize("name", ["R1", "R2", "R0", "R3"])
def test_reference_against_dense_spectrum(name):
    """Counts 3 / 13 / 0 / 59 inside by the dense spectrum; the restatement returns them one to one (R1, R2), nothing (R0: no Ritz
    value inside in either of its two iterations -- an empty region is declared only after a second one --, complete with spare
    directions) or reports the full subspace (R3: all 40 Ritz values inside,
    ``complete`` false).  R2 converges within ``max_it = 12``."""
    (centre, rx, ry, nodes, cols), count, complete = rr.REGIONS[name]
    A, M = rr.s2k()
    dense = rr.dense_spectrum()
    assert int(rr.inside(dense, centre, rx, ry).sum()) == count
    out = rr.contour_solve(A, M, centre, rx, ry, nodes, rr.start_block(A.shape[0], cols))
    print(name, "iterations", out.iterations, "history", out.inside_history, "estimate", out.estimate)
    assert out.complete == complete
    if name == "R3":
        assert out.count == cols and out.iterations == rr.MAX_IT and not np.any(out.residuals <= rr.ATOL)
        return
    assert out.count == count and np.all(out.residuals <= rr.ATOL) and out.iterations <= rr.MAX_IT
    if name == "R0":
        assert out.iterations == 2 and all(h[0] == 0 for h in out.inside_history)
    rr.assert_one_to_one(out.eigenvalues, dense, lambda z: rr.inside(z, centre, rx, ry), centre, rx, ry)
    r = A @ out.eigenvectors - (M @ out.eigenvectors) * out.eigenvalues
    assert np.all(np.linalg.norm(r, axis=0) <= 2 * rr.ATOL * (np.linalg.norm(A @ out.eigenvectors, axis=0)
                                                             + np.abs(out.eigenvalues) * np.linalg.norm(M @ out.eigenvectors, axis=0)))


@pytest.mark.parametrize("nodes", [8, 16])
def test_quadrature_of_the_cauchy_kernel(nodes):
    """``f(lam) = sum_k w_k / (z_k - lam)`` on a circle of radius ``r`` about ``c``.  With ``u = (lam - c) / r`` and the nodes
    ``z_k = c + r e^{i t_k}``, ``w_k = r e^{i t_k} / N``: ``f = (1/N) sum_k 1 / (1 - u e^{-i t_k})``.  For ``|u| = rho < 1`` the
    geometric series gives ``(1/N) sum_k sum_m u^m e^{-i m t_k}``; ``sum_k e^{-i m t_k}`` is ``N (-1)^j`` for ``m = j N`` (the half
    step) and 0 otherwise, so ``f = 1 / (1 + u^N)`` and ``|f - 1| <= rho^N / (1 - rho^N)``.  For ``rho > 1`` the series in ``1 / u``
    gives ``f = 1 - 1 / (1 + u^-N) = u^-N / (1 + u^-N)``: ``|f| <= rho^-N / (1 - rho^-N)``.  Rounding adds a few ulps."""
    c, r = 0.3 - 0.2j, 0.7
    z, w = contour_nodes(Ellipse(c, r, r), nodes)
    zr, wr = rr.nodes_and_weights(c, r, r, nodes)
    assert np.array_equal(z, zr) and np.array_equal(w, wr)
    assert np.all(z.imag != 0.0) or c.imag != 0.0
    assert np.all(contour_nodes(Ellipse(0.5, 1.0, 2.0), nodes)[0].imag != 0.0)  # no node on the real axis
    for rho in (0.0, 0.3, 0.8, 0.95):
        for phase in (0.0, 1.1, 2.9):
            f = np.sum(w / (z - (c + rho * r * np.exp(1j * phase))))
            assert abs(f - 1.0) <= rho**nodes / (1.0 - rho**nodes) + 1e-14
    for rho in (1.05, 1.5, 4.0):
        for phase in (0.0, 1.1, 2.9):
            f = np.sum(w / (z - (c + rho * r * np.exp(1j * phase))))
            assert abs(f) <= rho**-nodes / (1.0 - rho**-nodes) + 1e-14
    # an ellipse: the weights are dz/dt / (i N), so the rule still counts 1 inside and 0 far outside
    z, w = contour_nodes(Ellipse(c, 0.5, 1.5), 64)
    assert abs(np.sum(w / (z - c)) - 1.0) < 1e-8 and abs(np.sum(w / (z - (c + 6.0)))) < 1e-8


def test_rectangle_is_the_circumscribing_ellipse():
    rect = Rectangle(-0.05, 0.10, 0.65, 0.80)
    e = rect.ellipse()
    assert e.centre == pytest.approx(0.025 + 0.725j)
    assert e.rx == pytest.approx(np.sqrt(2.0) * 0.075) and e.ry == pytest.approx(np.sqrt(2.0) * 0.075)
    corners = np.array([-0.05 + 0.65j, 0.10 + 0.65j, -0.05 + 0.80j, 0.10 + 0.80j])
    c = complex(e.centre)
    assert ((corners.real - c.real) / e.rx) ** 2 + ((corners.imag - c.imag) / e.ry) ** 2 == pytest.approx(np.ones(4))  # corners on the ellipse
    pts = np.array([0.0 + 0.7j, -0.049 + 0.651j, -0.06 + 0.7j, 0.025 + 0.82j])
    assert rect.contains(pts).tolist() == [True, True, False, False]
    assert np.all(e.contains(pts[rect.contains(pts)]))  # the ellipse covers the rectangle
    assert e.contains(0.025 + 0.82j) and not rect.contains(0.025 + 0.82j)


def test_refusals_come_before_any_device_work():
    A, M = rr.s2k()
    with pytest.raises(ValueError, match="needs M"):
        RegionEigenSolver(A, None)
    with pytest.raises(ValueError, match="real M"):
        RegionEigenSolver(A, M.astype(np.complex128))
    with pytest.raises(NotImplementedError, match="one GPU"):
        RegionEigenSolver(A, M, layout="sharded")
    from Solver.utils import PreconditionerType

    with pytest.raises(NotImplementedError, match="exact LU"):
        RegionEigenSolver(A, M, pc_type=PreconditionerType.ILU)
    with pytest.raises(NotImplementedError, match="exact LU"):
        RegionEigenSolver(A, M, ilu_levels=1)
    for bad in (dict(nodes=3), dict(nodes=7), dict(nodes=2), dict(subspace=1), dict(subspace=129), dict(atol=0.0), dict(max_it=0), dict(keep_factors="yes")):
        with pytest.raises(ValueError, match=next(iter(bad))):
            RegionEigenSolver(A, M, RegionConfig(**bad))
    with pytest.raises(ValueError, match="exceeds the problem size"):
        RegionEigenSolver(A[:40, :40], M[:40, :40], RegionConfig(subspace=48))
    for bad in ((0.1, 0.0, 1.0), (0.1, 1.0, -1.0), (np.nan, 1.0, 1.0), (0.1, np.inf, 1.0)):
        with pytest.raises(ValueError, match="Ellipse"):
            Ellipse(*bad)
    for bad in ((0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 2.0, 1.0), (0.0, np.inf, 0.0, 1.0)):
        with pytest.raises(ValueError, match="Rectangle"):
            Rectangle(*bad)
    rs = RegionEigenSolver(A, M)
    with pytest.raises(ValueError, match="Ellipse or a Rectangle"):
        rs.solve((0.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="Y0 must have shape"):
        rs.solve(Ellipse(0.0, 1.0, 1.0), Y0=np.zeros((A.shape[0], 3)))
    assert np.array_equal(rs.start_block(), rr.start_block(A.shape[0], 48, 0))


def test_all_on_non_hermitian_problems_still_refuses():
    """``iEpsWhich.ALL`` on ``NHEP`` / ``GNHEP`` keeps raising: regions are :class:`RegionEigenSolver` 's."""
    from Solver.utils import iEpsProblemType, iEpsSolver, iEpsWhich

    A, M = rr.s2k()
    eps = iEpsSolver(A, M)
    eps.set_problem_type(iEpsProblemType.GNHEP)
    eps.set_which_eigenpairs(iEpsWhich.ALL)
    eps.set_interval_complex(-0.1, 0.1, 0.6, 0.8)
    with pytest.raises((ValueError, NotImplementedError)):
        eps.solve()


def test_symmetric_membrane_circle_on_the_real_axis():
    """The membrane pair (P2, 32 x 32 on [0, 2] x [0, 4]): the circle of radius 5 about 14 holds the five analytic eigenvalues
    10.49, the double 12.34, 15.42 and 17.89; the nearest ones outside are 8.02 and 19.74; all of them stay more than 10 % of the
    radius away from the contour.  (The circle first tried, radius 6 about 8, is the next test.)
    P2 elements with h = 1/16 .. 1/8 resolve these
    modes to a relative ``C h^4 lam`` well below 1e-3 (tests/golden/reference_known_answers.json: 2e-5 on average over the first 15)."""
    from synthetic import fem

    A, M, _ = fem.assemble_membrane(32, 32)
    ana = fem.membrane_analytic(12)
    centre, r = 14.0 + 0.0j, 5.0
    assert np.all(np.abs(np.abs(np.append(ana, 1.0) - centre.real) - r) >= 0.1 * r)
    want = ana[np.abs(ana - centre.real) < r]
    assert want.size == 5
    out = rr.contour_solve(A, M, centre, r, r, 16, rr.start_block(A.shape[0], 16))
    print("membrane: iterations", out.iterations, "history", out.inside_history)
    assert out.count == 5 and out.complete
    got = np.sort(out.eigenvalues.real)
    assert np.all(np.abs(out.eigenvalues.imag) <= 1e-8) and np.all(np.abs(got - want) <= 1e-3 * want)


def test_cluster_next_to_the_contour_does_not_empty_the_region():
    """The circle of radius 6 about 8 on the membrane pair holds six eigenvalues and passes at relative radius 1.17 of the Dirichlet
    rows' 248-fold ``lambda = 1``, whose directions fill the 16 columns of the first quadrature: iteration 1 shows NO Ritz value
    inside.  Stopping there would report an empty region as complete; the rule asks a second iteration to confirm an empty
    region, which shows all six, and the iteration goes on until they have converged (slowly: the cluster is filtered by 0.085 per
    iteration only)."""
    from synthetic import fem

    A, M, _ = fem.assemble_membrane(32, 32)
    want = fem.membrane_analytic(6)
    out = rr.contour_solve(A, M, 8.0 + 0.0j, 6.0, 6.0, 16, rr.start_block(A.shape[0], 16), max_it=20)
    print("membrane, cluster near the contour: iterations", out.iterations, "history", out.inside_history)
    assert out.inside_history[0] == (0, 0) and out.inside_history[1][0] == 6
    assert out.count == 6 and out.complete and np.all(np.abs(np.sort(out.eigenvalues.real) - want) <= 1e-3 * want)
