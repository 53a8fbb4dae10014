"""GPU tests of the left phase of the region eigensolver (``lsa_contour_solve_left``, ``RegionConfig(two_sided=True)``) on the S2k
regions of ``tests/region_reference.py``: the right phase untouched, left eigenvalues one to one with the right ones, biorthogonality
and left residuals recomputed on the host, ``kappa`` against the CPU restatement of ``tests/region_left_reference.py`` at the tolerance
``tests/test_region_left_cpu.py`` derives, and kept, refactorised and lockstep factor sets returning the same bytes."""

import logging
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_RESULTS = {}
LEFT_FIELDS = ("left_eigenvalues", "left_residuals_raw", "left_eigenvectors", "left_residuals", "condition_numbers")
RIGHT_FIELDS = ("eigenvalues", "eigenvectors", "residuals")


def _region(name):
    import region_reference as rr
    from Solver.region import Ellipse, RegionConfig

    (centre, rx, ry, nodes, cols), count, complete = rr.REGIONS[name]
    return Ellipse(centre, rx, ry), RegionConfig(nodes=nodes, subspace=cols, atol=rr.ATOL, max_it=rr.MAX_IT), count, complete


def _solve(name, two_sided=True, keep_factors=None, batch_nodes=False):
    """One fresh solver per (region, mode), kept for the module; the start block is the CPU test's."""
    import region_reference as rr
    from Solver.region import RegionEigenSolver

    key = (name, two_sided, keep_factors, batch_nodes)
    if key not in _RESULTS:
        ell, cfg, _, _ = _region(name)
        A, M = rr.s2k()
        rs = RegionEigenSolver(A, M, replace(cfg, keep_factors=keep_factors, batch_nodes=batch_nodes, two_sided=two_sided))
        try:
            _RESULTS[key] = rs.solve(ell, Y0=rr.start_block(A.shape[0], cfg.subspace))
        finally:
            rs.release()
    return _RESULTS[key]


def _same(a, b, fields):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in fields)


@pytest.mark.parametrize("name", ["R1", "R2", "R0"])
def test_two_sided_leaves_the_right_phase_untouched(name):
    """``two_sided=True`` returns the bytes of ``two_sided=False`` in every field the right phase fills, and the same counters; with
    ``two_sided=False`` the left fields are ``None`` and ``stats`` has no ``"left"``."""
    one, two = _solve(name, two_sided=False), _solve(name)
    assert _same(one, two, RIGHT_FIELDS)
    assert (one.count, one.complete, one.iterations, one.estimate) == (two.count, two.complete, two.iterations, two.estimate)
    for key, value in one.stats.items():
        if not key.startswith("seconds_") and key != "analysis_reused":
            assert two.stats[key] == value, key
    assert "left" not in one.stats and one.left_complete is None and all(getattr(one, f) is None for f in LEFT_FIELDS)
    left = two.stats["left"]
    assert left["iterations"] >= 1 and left["block_solves"] > 0 and left["seconds_solve"] > 0.0


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_left_eigenpairs_and_condition_numbers(name):
    import region_left_reference as lref
    import region_reference as rr
    KAPPA_RTOL = lref.KAPPA_RTOL

    ell, cfg, count, _ = _region(name)
    res = _solve(name)
    A, M = rr.s2k()
    assert res.count == count and res.left_complete is True
    # one to one with the right eigenvalues (the rule of the CPU test)
    lam, llam = res.eigenvalues, res.left_eigenvalues
    nearest = np.argmin(np.abs(llam[:, None] - lam[None, :]), axis=1)
    dist = np.abs(llam - lam[nearest])
    assert llam.size == count and len(set(nearest.tolist())) == count
    assert dist.max() <= rr.match_tolerance(rr.dense_spectrum(), complex(ell.centre), ell.rx, ell.ry)
    assert np.all(res.left_residuals_raw <= cfg.atol)
    # biorthogonality and left residuals recomputed on the host
    W, X = res.left_eigenvectors, res.eigenvectors
    assert W.shape == X.shape == (A.shape[0], count)
    off = np.abs(W.conj().T @ (M @ X) - np.eye(count)).max()
    host = lref.left_residuals(A, M, lam, W)
    print(f"{name}: |W^H M X - I| max {off:.2e}; left residuals device max {res.left_residuals.max():.3e}, host max {host.max():.3e}")
    assert off <= 1e-10
    assert np.all(host <= 2 * cfg.atol) and np.all(res.left_residuals <= 2 * cfg.atol)
    assert np.allclose(res.left_residuals, host, rtol=0.1, atol=1e-13)
    # kappa against the CPU restatement: its own right and left phases, biorthonormalised; matched through the eigenvalues
    (centre, rx, ry, nodes, cols), _, _ = rr.REGIONS[name]
    Y0 = rr.start_block(A.shape[0], cols)
    right = rr.contour_solve(A, M, centre, rx, ry, nodes, Y0)
    left = lref.left_solve(A, M, centre, rx, ry, nodes, Y0)
    _, _, kref = lref.biorthonormalise(M, right.eigenvectors, left.eigenvectors)
    at = np.argmin(np.abs(lam[:, None] - right.eigenvalues[None, :]), axis=1)
    assert len(set(at.tolist())) == count
    dev = np.abs(res.condition_numbers - kref[at]) / kref[at]
    print(f"{name}: kappa {res.condition_numbers.min():.3e} .. {res.condition_numbers.max():.3e}; deviation from the CPU reference max {dev.max():.3e} (allowed {KAPPA_RTOL:.1e})")
    assert np.all(dev <= KAPPA_RTOL)


def test_empty_region_is_left_complete_with_zero_columns():
    res = _solve("R0")
    assert res.count == 0 and res.left_complete is True
    assert res.left_eigenvalues.size == 0 and res.left_eigenvectors.shape == (1953, 0)
    assert res.left_residuals.size == 0 and res.condition_numbers.size == 0


def test_kept_refactorised_and_lockstep_give_the_same_bytes():
    kept, refac, batch = _solve("R2", keep_factors=True), _solve("R2", keep_factors=False), _solve("R2", keep_factors=True, batch_nodes=True)
    assert kept.stats["factors_kept"] is True and refac.stats["factors_kept"] is False and batch.stats["batch_nodes"] is True
    for other in (refac, batch):
        assert _same(kept, other, RIGHT_FIELDS + LEFT_FIELDS)
        assert other.left_complete is True and other.stats["left"]["iterations"] == kept.stats["left"]["iterations"]
    assert kept.stats["left"]["batched_columns"] == 0 and refac.stats["left"]["batched_columns"] == 0
    assert batch.stats["left"]["batched_columns"] > 0 and batch.stats["left"]["batched_groups"] > 0
    # the right phase's counters do not hold the left phase's: those of a right-only solve in the same mode
    alone = _solve("R2", two_sided=False, keep_factors=True, batch_nodes=True)
    assert alone.stats["batched_columns"] == batch.stats["batched_columns"] and alone.stats["block_solves"] == batch.stats["block_solves"]


def test_full_left_subspace_is_reported(caplog):
    """R3: 59 eigenvalues inside, 40 columns: neither phase completes; ``left_complete`` is false, the three derived fields stay ``None``
    and a warning says which condition failed."""
    import region_reference as rr
    from Solver.region import RegionEigenSolver

    ell, cfg, _, _ = _region("R3")
    A, M = rr.s2k()
    rs = RegionEigenSolver(A, M, replace(cfg, two_sided=True))
    try:
        with caplog.at_level(logging.WARNING, logger="Solver.region"):
            res = rs.solve(ell, Y0=rr.start_block(A.shape[0], cfg.subspace))
    finally:
        rs.release()
    assert not res.complete and res.left_complete is False
    assert res.left_eigenvectors is None and res.left_residuals is None and res.condition_numbers is None
    assert res.left_eigenvalues is not None and res.left_residuals_raw is not None
    left = res.stats["left"]
    assert left["iterations"] == cfg.max_it and left["converged_inside"] < left["inside_ellipse"] and left["inside_ellipse"] >= cfg.subspace - 1
    assert any("no left eigenvectors" in r.getMessage() and "did not complete" in r.getMessage() for r in caplog.records)
