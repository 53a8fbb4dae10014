"""CPU suite: the left phase of the region eigensolver as restated in ``region_left_reference.py`` on the S2k regions with 3 (R1) and 13
(R2) eigenvalues inside, the front end's configuration, and the binding's new names.

Measured here (printed by ``test_left_phase_and_condition_numbers``): the relative deviation of ``kappa_i`` between the restatement
(contour iteration + biorthonormalisation) and inverse iteration with ``splu((A - (lam_i + delta) M)^H)`` is 2.3e-10 on R1
and 9.2e-10 on R2 (two, three and four steps of inverse iteration give the same figure to two digits: it is the restatement's own
error, the left residual 2e-11 times ``kappa`` of 6 .. 33), recorded as ``region_left_reference.KAPPA_DEVIATION`` = 1e-9.  The GPU test allows ten times
that (``KAPPA_RTOL``): another summation order moves ``w`` by the left residual times ``kappa``; the assertion here allows the same
ten times, since another BLAS or SuperLU build is another summation order too."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import region_left_reference as lref
import region_reference as rr

HEADER = Path(__file__).resolve().parents[1] / "include" / "lsa_hip.h"
KAPPA_RTOL = lref.KAPPA_RTOL  # ten times the deviation measured below; what tests/test_gpu_region_left.py allows too

_RUNS = {}


def run(name):
    """Right and left restatement of region ``name`` from the same start block, once per session."""
    if name not in _RUNS:
        A, M = rr.s2k()
        (centre, rx, ry, nodes, cols), _, _ = rr.REGIONS[name]
        Y0 = rr.start_block(A.shape[0], cols)
        right = rr.contour_solve(A, M, centre, rx, ry, nodes, Y0)
        left = lref.left_solve(A, M, centre, rx, ry, nodes, Y0)
        _RUNS[name] = (right, left)
    return _RUNS[name]


def test_left_quadrature_is_the_adjoint_pencils_projector():
    """The sign and the conjugation: ``-sum_k conj(w_k) C_k^-H M^H Y`` on the factors of ``C_k`` equals, to rounding, the right-phase
    quadrature ``-sum_j w'_j (A^H - z'_j M^H)^-1 M^H Y`` written out on the adjoint pencil's OWN nodes and weights on the conjugate
    ellipse with its own factorisations; flipping the sign or dropping the conjugation of the weights does not."""
    import scipy.sparse.linalg as spla

    A, M = rr.s2k()
    (centre, rx, ry, nodes, cols), _, _ = rr.REGIONS["R1"]
    AH, MH = sp.csr_matrix(A.conj().T), sp.csr_matrix(M.conj().T)
    Y = rr.start_block(A.shape[0], cols)
    z, w = rr.nodes_and_weights(centre, rx, ry, nodes)
    lus = [spla.splu((A - zk * M).tocsc()) for zk in z]
    Q = lref.left_quadrature(lus, w, MH, Y)
    z2, w2 = rr.nodes_and_weights(np.conj(centre), rx, ry, nodes)
    own = sum(-wk * spla.splu((AH - zk * MH).tocsc()).solve(MH @ Y) for zk, wk in zip(z2, w2))
    scale = np.linalg.norm(own)
    assert np.linalg.norm(Q - own) <= 1e-9 * scale
    B = MH @ Y
    unconjugated = sum(-wk * lu.solve(B, trans="H") for wk, lu in zip(w, lus))
    assert np.linalg.norm(-Q - own) > 0.5 * scale and np.linalg.norm(unconjugated - own) > 1e-3 * scale


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_left_phase_and_condition_numbers(name):
    A, M = rr.s2k()
    (centre, rx, ry, nodes, cols), count, complete = rr.REGIONS[name]
    right, left = run(name)
    assert right.count == count and left.count == count and left.complete and right.complete
    # one to one: every left eigenvalue on a right one, none taken twice
    nearest = np.argmin(np.abs(left.eigenvalues[:, None] - right.eigenvalues[None, :]), axis=1)
    dist = np.abs(left.eigenvalues - right.eigenvalues[nearest])
    assert len(set(nearest.tolist())) == count and dist.max() <= rr.match_tolerance(rr.dense_spectrum(), centre, rx, ry)
    assert np.all(left.residuals <= rr.ATOL)
    Wb, G, kappa = lref.biorthonormalise(M, right.eigenvectors, left.eigenvectors)
    MX = M @ right.eigenvectors
    I = Wb.conj().T @ MX
    off = np.abs(I - np.eye(count)).max()
    res = lref.left_residuals(A, M, right.eigenvalues, Wb)
    ref = np.array([lref.kappa_by_inverse_iteration(A, M, lam, right.eigenvectors[:, i]) for i, lam in enumerate(right.eigenvalues)])
    dev = np.abs(kappa - ref) / ref
    print(f"{name}: |W^H M X - I| max {off:.2e}; left residuals max {res.max():.2e}; kappa {kappa.min():.3e} .. {kappa.max():.3e}; "
          f"relative deviation from inverse iteration max {dev.max():.3e}")
    assert off <= 1e-10
    assert np.all(res <= rr.ATOL)
    assert np.all(dev <= KAPPA_RTOL)


def test_region_config_validates_two_sided():
    from Solver.region import RegionConfig, RegionResult, _check_config

    cfg = RegionConfig()
    assert cfg.two_sided is False
    _check_config(RegionConfig(two_sided=True))
    _check_config(RegionConfig(two_sided=True, batch_nodes=True, keep_factors=True))
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="two_sided"):
            _check_config(RegionConfig(two_sided=bad))
    r = RegionResult(np.zeros(0), np.zeros((3, 0)), np.zeros(0), 0, True, 0.0, 1)
    for name in ("left_eigenvalues", "left_residuals_raw", "left_complete", "left_eigenvectors", "left_residuals", "condition_numbers"):
        assert getattr(r, name) is None
    assert "left" not in r.stats


def test_left_phase_symbols_declared_exported_and_bound():
    import lsa_hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = lsa_hip.load_library()
    for name in ("lsa_contour_solve_left", "lsa_contour_left_info"):
        assert re.search(rf"\b{name}\s*\(", text) and hasattr(lib, name) and name in lsa_hip.SIGNATURES
    assert lsa_hip.SIGNATURES["lsa_contour_solve_left"] == lsa_hip.SIGNATURES["lsa_contour_solve"]
    fields = [name for name, _ in lsa_hip.lsa_contour_left_stats._fields_]
    struct = re.search(r"typedef struct \{([^}]*)\} lsa_contour_left_stats;", text).group(1)
    assert fields == re.findall(r"(\w+);", struct)
    assert ctypes.sizeof(lsa_hip.lsa_contour_left_stats) == 2 * 4 + 6 * 8 + 5 * 8
    assert hasattr(lsa_hip.ContourSolver, "solve_left") and hasattr(lsa_hip.ContourSolver, "left_info")
