"""GPU tests of the region eigensolver (``csrc/contour.hip``, ``Solver/region.py``) on the S2k cylinder case (n = 1953, no multiple
of any tile): the multi-column SpMV ``lsa_spmm`` and the deterministic block Gram ``lsa_block_gram`` driven directly on ``lsa_vec``
blocks, then ``RegionEigenSolver`` on the regions of ``tests/region_reference.py`` against the dense spectrum of the pencil.

Bounds.  With ``eps = 2^-53`` and ``gamma_k = k eps / (1 - k eps)``:

* a sum of ``k`` products accumulated in ANY order by fused multiply-adds is within ``gamma_k sum |a_i| |x_i|`` of the exact sum
  (Higham, Accuracy and Stability, section 3.1: no path through the summation tree is longer than ``k`` roundings).  A row of the
  SpMV with ``len`` entries is far shorter than that in the kernel (``len / 8`` per lane, then three tree levels), and the scipy
  product it is compared with carries its own ``gamma_len``; ``k = longest row + 2`` covers both a complex product's two terms
  per part and the comparison.
* the Gram entry ``(i, j)`` is a sum over ``n`` rows: ``gamma_(n+2) (|U|^H |W|)_ij``.
"""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
Z = 0.018 + 0.7379601143282424j  # the bench shift: C = A - Z M is complex
PAD = 3                          # leading dimension n + PAD

_CASE = {}


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def _s2k(hip_ctx):
    """Host and device copies of M (real) and C = A - Z M (complex) of S2k, uploaded once for the module."""
    import lsa_hip
    from synthetic import fem

    if not _CASE:
        es = fem.cylinder_case("S2k")
        M = sp.csr_matrix(es.M)
        C = sp.csr_matrix((es.A.data - Z * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
        for m in (M, C):
            m.sort_indices()
        assert M.dtype == np.float64 and C.dtype == np.complex128 and M.shape[0] == 1953
        _CASE.update(n=M.shape[0], M=M, C=C, dM=lsa_hip.CsrMatrix.from_scipy(hip_ctx, M), dC=lsa_hip.CsrMatrix.from_scipy(hip_ctx, C))
    return _CASE


def _block(n, cols, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols)))


def _upload_block(hip_ctx, B, ld, fill=np.nan):
    """The block as one device vector of ``ld * cols`` entries, the rows behind row n of every column holding ``fill``."""
    import lsa_hip

    n, cols = B.shape
    flat = np.full((ld, cols), fill, dtype=np.complex128, order="F")
    flat[:n] = B
    return lsa_hip.DeviceVector.from_numpy(hip_ctx, flat.reshape(-1, order="F"))


@pytest.mark.parametrize("operand", ["M-real", "C-complex"])
@pytest.mark.parametrize("cols", [1, 7, 8, 9, 17])
def test_spmm_against_scipy(hip_ctx, operand, cols):
    """``Y = A X`` for a pass remainder (1, 7), one full pass (8), a pass and a remainder (9) and two passes and one (17), with
    ``ld = n + 3``: componentwise within ``gamma_k (|A| |X|)``, ``k`` = longest row + 2; the rows between the columns untouched (and
    never read: they hold NaN in X); two calls give the same bytes."""
    import lsa_hip

    s = _s2k(hip_ctx)
    n, ld = s["n"], s["n"] + PAD
    A, dA = (s["M"], s["dM"]) if operand == "M-real" else (s["C"], s["dC"])
    X = _block(n, cols, seed=cols)
    dX = _upload_block(hip_ctx, X, ld)
    outs = []
    for _ in range(2):
        dY = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(ld * cols, 7.0 - 5.0j))
        dA.matmat(dX, dY, cols, ldx=ld, ldy=ld)
        outs.append(dY.numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    Y = outs[0].reshape((ld, cols), order="F")
    assert np.all(Y[n:] == 7.0 - 5.0j), "rows between the columns were written"
    ref = A @ X
    k = int(np.diff(A.indptr).max()) + 2
    bound = gamma(k) * (abs(A) @ np.abs(X))
    err = np.abs(Y[:n] - ref)
    print(f"spmm {operand} cols={cols}: k={k}, max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.isfinite(Y[:n])) and np.all(err <= bound)


@pytest.mark.parametrize("q", [1, 8, 48, 128])
@pytest.mark.parametrize("p", [1, 8, 48, 128])
def test_block_gram_against_numpy(hip_ctx, p, q):
    """``G = U^H W`` over n = 1953 rows (two row chunks; p and q below, at and above the 4 x 4 tile): componentwise within
    ``gamma_(n+2) (|U|^H |W|)``, two calls the same bytes; ``G(U, U)`` Hermitian to that bound with an exactly real diagonal."""
    import lsa_hip

    n = 1953
    ldu, ldw = n + PAD, n
    U, W = _block(n, p, seed=100 + p), _block(n, q, seed=200 + q)
    dU, dW = _upload_block(hip_ctx, U, ldu), _upload_block(hip_ctx, W, ldw)
    G = lsa_hip.block_gram(hip_ctx, n, dU, p, dW, q, ldu=ldu, ldw=ldw)
    G2 = lsa_hip.block_gram(hip_ctx, n, dU, p, dW, q, ldu=ldu, ldw=ldw)
    assert G.shape == (p, q) and G.tobytes() == G2.tobytes()
    bound = gamma(n + 2) * (np.abs(U).T @ np.abs(W))
    err = np.abs(G - U.conj().T @ W)
    print(f"gram p={p} q={q}: max err / bound = {np.max(err / bound):.4f}")
    assert np.all(np.isfinite(G)) and np.all(err <= bound)
    if q == p:
        S = lsa_hip.block_gram(hip_ctx, n, dU, p, dU, p, ldu=ldu, ldw=ldu)
        sbound = gamma(n + 2) * (np.abs(U).T @ np.abs(U))
        assert np.all(np.abs(S - U.conj().T @ U) <= sbound)
        assert np.all(np.abs(S - S.conj().T) <= sbound)
        assert np.all(np.diag(S).imag == 0.0) and np.all(np.diag(S).real > 0.0)


def test_block_arguments_are_refused(hip_ctx):
    """Blocks that do not fit their vectors, real blocks, aliasing and sizes beyond 128 columns: ``LSA_ERR_ARG`` with the condition
    named, before any launch."""
    import lsa_hip

    s = _s2k(hip_ctx)
    n = s["n"]
    x = lsa_hip.DeviceVector(hip_ctx, 2 * n)
    y = lsa_hip.DeviceVector(hip_ctx, 2 * n)
    with pytest.raises(ValueError, match="does not fit"):
        s["dM"].matmat(x, y, 3)                      # three columns in vectors of two
    with pytest.raises(ValueError, match="does not fit"):
        s["dM"].matmat(x, y, 2, ldx=n - 1, ldy=n)    # ld < n
    with pytest.raises(ValueError, match="alias"):
        s["dM"].matmat(x, x, 2)
    with pytest.raises(ValueError, match="complex128"):
        s["dM"].matmat(lsa_hip.DeviceVector(hip_ctx, n, np.float64), y, 1)
    with pytest.raises(ValueError, match="between 1 and 128"):
        lsa_hip.block_gram(hip_ctx, 4, lsa_hip.DeviceVector(hip_ctx, 4 * 129), 129, lsa_hip.DeviceVector(hip_ctx, 4), 1)
    with pytest.raises(ValueError, match="do not fit"):
        lsa_hip.block_gram(hip_ctx, n, x, 2, y, 3)
    with pytest.raises(ValueError, match="complex128"):
        lsa_hip.block_gram(hip_ctx, n, lsa_hip.DeviceVector(hip_ctx, n, np.float64), 1, y, 1)


# ---- the iteration: RegionEigenSolver on the regions of region_reference against the dense spectrum --------------------------------

_RESULTS = {}


def _region(name):
    from Solver.region import Ellipse, RegionConfig
    import region_reference as rr

    (centre, rx, ry, nodes, cols), count, complete = rr.REGIONS[name]
    return Ellipse(centre, rx, ry), RegionConfig(nodes=nodes, subspace=cols, atol=rr.ATOL, max_it=rr.MAX_IT), count, complete


def _solve(name, keep_factors=None):
    """One fresh solver per (region, factor mode), kept for the module; the start block is the CPU test's."""
    from dataclasses import replace

    from Solver.region import RegionEigenSolver
    import region_reference as rr

    key = (name, keep_factors)
    if key not in _RESULTS:
        ell, cfg, _, _ = _region(name)
        A, M = rr.s2k()
        rs = RegionEigenSolver(A, M, replace(cfg, keep_factors=keep_factors))
        try:
            _RESULTS[key] = rs.solve(ell, Y0=rr.start_block(A.shape[0], cfg.subspace))
        finally:
            rs.release()
    return _RESULTS[key]


def _same_bytes(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("eigenvalues", "eigenvectors", "residuals")) and \
        (a.count, a.complete, a.iterations, a.estimate) == (b.count, b.complete, b.iterations, b.estimate)


def _check_pairs(res, region_mask, centre, rx, ry, atol, pencil=None, dense=None):
    """Eigenvalues one to one with the dense ones in the region (the CPU rule), residuals recomputed on the host within ``2 atol``
    (the factor covers another summation order and nothing else), unit 2-norm, canonical phase.  ``pencil``, ``dense``: S2k's
    unless given."""
    import region_reference as rr

    A, M = rr.s2k() if pencil is None else pencil
    rr.assert_one_to_one(res.eigenvalues, rr.dense_spectrum() if dense is None else dense, region_mask, centre, rx, ry)
    X, lam = res.eigenvectors, res.eigenvalues
    assert X.shape == (A.shape[0], res.count)
    if res.count == 0:
        return
    AX, MX = A @ X, M @ X
    host = np.linalg.norm(AX - MX * lam, axis=0) / (np.linalg.norm(AX, axis=0) + np.abs(lam) * np.linalg.norm(MX, axis=0))
    print(f"residuals: device max {res.residuals.max():.3e}, host max {host.max():.3e}")
    assert np.all(host <= 2 * atol) and np.all(res.residuals <= atol)
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-13)
    big = X[np.argmax(np.abs(X), axis=0), np.arange(res.count)]
    assert np.all(big.real > 0) and np.all(np.abs(big.imag) <= 1e-14)


@pytest.mark.parametrize("name", ["R1", "R2", "R0"])
def test_regions_against_dense_spectrum(name):
    import region_reference as rr

    ell, cfg, count, complete = _region(name)
    res = _solve(name)
    print(name, "iterations", res.iterations, "estimate", res.estimate, "stats", res.stats)
    assert res.count == count and res.complete == complete and res.iterations <= rr.MAX_IT
    _check_pairs(res, ell.contains, complex(ell.centre), ell.rx, ell.ry, cfg.atol)
    assert res.stats["block_solves"] > 0
    assert res.iterations == {"R1": 3, "R2": 5, "R0": 2}[name]  # those of the numpy restatement (R0: the confirming second one)
    assert res.stats["max_rel_res"] <= 1e-8


def test_full_subspace_is_reported(caplog):
    """R3: 59 eigenvalues inside, 40 columns: all Ritz values stay inside, none converges, ``complete`` is false and the warning names
    the full subspace."""
    import logging

    import region_reference as rr
    from Solver.region import RegionEigenSolver

    ell, cfg, _, _ = _region("R3")
    A, M = rr.s2k()
    rs = RegionEigenSolver(A, M, cfg)
    try:
        with caplog.at_level(logging.WARNING, logger="Solver.region"):
            res = rs.solve(ell, Y0=rr.start_block(A.shape[0], cfg.subspace))
    finally:
        rs.release()
    assert not res.complete and res.iterations == cfg.max_it and res.stats["inside_ellipse"] == res.stats["rank"] == cfg.subspace
    assert any("subspace is full" in r.getMessage() and "raise `subspace`" in r.getMessage() for r in caplog.records)


def test_kept_and_refactorised_factors_give_the_same_bytes():
    kept, refac, again = _solve("R1", True), _solve("R1", False), None
    assert kept.stats["factors_kept"] is True and refac.stats["factors_kept"] is False
    assert _same_bytes(kept, refac)
    _RESULTS.pop(("R1", True))
    again = _solve("R1", True)  # a second, identical solve on a fresh solver
    assert _same_bytes(kept, again)
    assert _same_bytes(kept, _solve("R1"))  # (whichever mode the free memory chose)


def test_rectangle_is_filtered_from_the_ellipse():
    """A rectangle inscribed in R2's circle: the contour is R2's circle itself (half-widths r / sqrt 2), so the result is the
    subset of R2's pairs inside the rectangle; the count agrees with the dense set and ``complete`` holds.  The semi-axes
    ``sqrt(2) (r / sqrt(2))`` round to a neighbour of ``r`` and the centre is recomputed from the corners, so nodes and weights differ
    from R2's in their last bits and the pairs cannot be byte-equal to test 3's: they are compared as eigenpairs (1e-9 on the
    eigenvalue, 1e-6 on the vectors' alignment; both far above the 1e-10 residuals, far below the eigenvalues' separation).  Byte
    equality of repeated runs is what ``test_kept_and_refactorised_factors_give_the_same_bytes`` and the sweep test pin."""
    import region_reference as rr
    from Solver.region import Rectangle, RegionEigenSolver

    ell, cfg, _, _ = _region("R2")
    c, hw = complex(ell.centre), ell.rx / np.sqrt(2.0)
    rect = Rectangle(c.real - hw, c.real + hw, c.imag - hw, c.imag + hw)
    A, M = rr.s2k()
    rs = RegionEigenSolver(A, M, cfg)
    try:
        res = rs.solve(rect, Y0=rr.start_block(A.shape[0], cfg.subspace))
    finally:
        rs.release()
    dense = rr.dense_spectrum()
    assert res.complete and res.count == int(rect.contains(dense).sum()) and 0 < res.count
    e = rect.ellipse()
    _check_pairs(res, rect.contains, complex(e.centre), e.rx, e.ry, cfg.atol)
    full = _solve("R2")
    for lam, x in zip(res.eigenvalues, res.eigenvectors.T):
        j = int(np.argmin(np.abs(full.eigenvalues - lam)))
        assert abs(full.eigenvalues[j] - lam) <= 1e-9 and abs(abs(np.vdot(full.eigenvectors[:, j], x)) - 1.0) <= 1e-6


def test_sweep_equals_fresh_solvers():
    import region_reference as rr
    from Solver.region import RegionConfig, RegionEigenSolver

    # one configuration for both regions (R2's: 16 nodes, 48 columns), the same start block
    cfg = RegionConfig(nodes=16, subspace=48, atol=rr.ATOL, max_it=rr.MAX_IT)
    A, M = rr.s2k()
    Y0 = rr.start_block(A.shape[0], cfg.subspace)
    ells = [_region(name)[0] for name in ("R1", "R2")]
    rs = RegionEigenSolver(A, M, cfg)
    try:
        swept = rs.sweep(ells, Y0)
    finally:
        rs.release()
    assert swept[1].stats["analysis_reused"] is True
    for ell, got in zip(ells, swept):
        fresh_solver = RegionEigenSolver(A, M, cfg)
        try:
            fresh = fresh_solver.solve(ell, Y0)
        finally:
            fresh_solver.release()
        assert _same_bytes(got, fresh)
    assert swept[0].count == 3 and swept[1].count == 13 and swept[0].complete and swept[1].complete


def _diagonal_pair(hip_ctx, n=24, singular=False, complex_m=False):
    import lsa_hip

    a = np.arange(1.0, n + 1.0)
    m = np.ones(n)
    if singular:
        a[5] = m[5] = 0.0  # a row of zeros in both (kept as explicit entries): every A - z M is singular
    A = sp.csr_matrix((a, np.arange(n), np.arange(n + 1)), shape=(n, n))
    M = sp.csr_matrix((m.astype(np.complex128) if complex_m else m, np.arange(n), np.arange(n + 1)), shape=(n, n))
    return lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)


def test_contour_create_refuses_by_name(hip_ctx):
    """``lsa_contour_create`` itself (the Python front end catches most of these first): ``LSA_ERR_ARG`` naming the condition."""
    import lsa_hip

    dA, dM = _diagonal_pair(hip_ctx)
    ok = dict(nodes=8, centre=3.5 + 0.0j, rx=1.0, ry=1.0, subspace=4)

    def create(A=dA, M=dM, **kw):
        a = {**ok, **kw}
        return lsa_hip.ContourSolver(hip_ctx, A, M, a["nodes"], a["centre"], a["rx"], a["ry"], a["subspace"])

    for kw, text in ((dict(nodes=2), "even number of at least 4"), (dict(nodes=7), "even number of at least 4"), (dict(subspace=1), "between 2 and"),
                     (dict(subspace=129), "between 2 and"), (dict(subspace=25), "between 2 and"), (dict(rx=0.0), "finite and positive"),
                     (dict(ry=-1.0), "finite and positive"), (dict(centre=complex(np.nan, 0.0)), "finite and positive")):
        with pytest.raises(ValueError, match=text):
            create(**kw)
    with pytest.raises(ValueError, match="M is missing"):
        create(M=None)
    with pytest.raises(ValueError, match="M is complex"):
        create(M=_diagonal_pair(hip_ctx, complex_m=True)[1])
    with pytest.raises(ValueError, match="do not share one pattern"):
        create(M=_s2k(hip_ctx)["dM"])
    cs = create()  # the accepted arguments do build, and find the eigenvalues 3 and 4 of the diagonal pencil
    out = cs.solve(1e-10, 10, _block(24, 4, seed=5))
    assert out["complete"] and sorted(np.round(out["eigenvalues"].real, 8).tolist()) == [3.0, 4.0]


def test_singular_node_is_a_zero_pivot_with_its_index(hip_ctx):
    """A pencil that is singular at a node (here at every node: a zero row in A and M) surfaces as ``LSA_ERR_ZERO_PIVOT`` naming node 0."""
    import lsa_hip

    dA, dM = _diagonal_pair(hip_ctx, singular=True)
    with pytest.raises(lsa_hip.LsaError, match=r"LSA_ERR_ZERO_PIVOT.*node 0 ") as exc:
        lsa_hip.ContourSolver(hip_ctx, dA, dM, 8, 3.5 + 0.0j, 1.0, 1.0, 4)
    assert exc.value.status == lsa_hip.LSA_ERR_ZERO_PIVOT


def test_s5k_region_spans_several_column_passes():
    """S5k (n = 4851: no multiple of 32, 256 or 1024; five row chunks) with 40 columns: five 8-column product passes, ten 4-column
    solve passes, 10 x 10 Gram tiles.  The region (``tests/golden/region_s5k.json``, written by ``make_golden_region_s5k.py`` from the
    dense spectrum of the pencil) is the circle of radius 0.0204 about -0.08 + 0.45j: 13 dense eigenvalues inside, so 27 spare
    directions, and the 41st nearest eigenvalue at 0.045377, beyond twice the radius (the numpy restatement converges at
    iteration 3, within 1.4e-11 of the dense values).  The
    checks are those of ``test_regions_against_dense_spectrum``."""
    import json
    from pathlib import Path

    import region_reference as rr
    from Solver.region import Ellipse, RegionConfig, RegionEigenSolver
    from synthetic import fem

    g = json.loads((Path(__file__).resolve().parent / "golden" / "region_s5k.json").read_text())
    centre, r, cols, count = complex(*g["centre"]), g["radius"], g["subspace"], g["count"]
    dense = np.array([complex(*z) for z in g["dense_within_3_radii"]])
    assert cols - count >= 12 and g["distance_of_subspace_plus_first"] > 2 * r and int(np.sum(np.abs(dense - centre) < r)) == count
    es = fem.cylinder_case("S5k")
    A, M = sp.csr_matrix(es.A), sp.csr_matrix(es.M)
    assert A.shape[0] == g["n"]
    ell, cfg = Ellipse(centre, r, r), RegionConfig(nodes=g["nodes"], subspace=cols, atol=rr.ATOL, max_it=rr.MAX_IT)
    rs = RegionEigenSolver(A, M, cfg)
    try:
        res = rs.solve(ell, Y0=rr.start_block(A.shape[0], cols))
    finally:
        rs.release()
    print("S5k iterations", res.iterations, "estimate", res.estimate, "stats", res.stats)
    assert res.count == count and res.complete and res.iterations <= rr.MAX_IT
    _check_pairs(res, ell.contains, centre, r, r, cfg.atol, pencil=(A, M), dense=dense)
    # (a node of this contour lies close to an eigenvalue -- the estimate of the count is useless here, -1163 --: every solve of the
    #  run carries the refinement step and about one in sixteen is accepted on its backward error, as the rule provides)
    assert res.stats["block_solves"] > 0 and res.stats["block_solves"] % res.stats["nodes"] == 0 and res.stats["max_rel_res"] <= 1e-8
