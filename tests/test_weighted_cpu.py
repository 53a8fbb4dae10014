"""CPU suite of the windowed / weighted analyses: the host references of ``tests/weighted_reference.py`` pinned (the restated weighted
iteration against the dense gains, ``weighted`` against scipy's product), every refusal of the front ends before any device work, the
result dataclasses' positional order, and the order in which ``ResolventSolver.norm_map`` visits its points.  The GPU suite
(``tests/test_gpu_weighted.py``) holds the library to the bounds these restatements meet."""

import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import growth_reference as gref
import growth_sdirk_reference as sref
import resolvent_reference as rref
import weighted_reference as ref


@pytest.mark.parametrize("key", list(ref.GAINS), ids=lambda k: f"beta{k[0]}-omega{k[1]:.2f}-{'f' if k[2] else 'M'}-{'q' if k[3] else 'M'}")
def test_restated_iteration_against_dense(key):
    """S2k, nev 4, ncv 12, tol 1e-10: the dense gains are the listed six decimals, the restated weighted iteration matches them to
    1e-12 sigma_1, restarts, and its pairs are orthonormal in their weights with R Qf f_j = sigma_j q_j."""
    beta, omega, fbox, qbox = key
    A, M = ref.case("S2k")
    Qf, Qq = ref.weight_of("S2k", fbox), ref.weight_of("S2k", qbox)
    dense = ref.dense_gains("S2k", beta, omega, fbox, qbox)[:4]
    assert np.allclose(dense, np.array(ref.GAINS[key]), rtol=0.0, atol=1e-6)
    shift = complex(beta, omega)
    out = ref.resolvent_trl(A, M, shift, 4, 12, 1e-10, rref.start_vector(A.shape[0]), Qf, Qq)
    oq, of, res = ref.pair_checks(A, M, shift, out["gains"], out["Q"], out["F"], Qf, Qq)
    err = np.abs(out["gains"] - dense).max() / dense[0]
    print(f"{key}: {out['restarts']} restarts, |gain - dense|_max / sigma_1 = {err:.2e}, |Q^H Qq Q - I| = {oq:.2e}, |F^H Qf F - I| = {of:.2e}, "
          f"pair residual = {res:.2e}")
    assert len(out["gains"]) == 4 and err <= 1e-12
    assert 1 <= out["restarts"] <= 12
    assert oq <= 1e-10 and of <= 1e-10 and res <= 1e-8


def test_forcing_region_and_real_shift():
    """The forcing region holds 90 velocity dofs with mass; the plain real shift z = 0.2 has the listed dense gains."""
    _, M = ref.case("S2k")
    d = ref.window("S2k", *ref.OMEGA_F)
    assert int((((d * M.diagonal()) * d) > 0.0).sum()) == 90
    from synthetic import fem

    for mine, theirs in zip(ref.dof_xy("S2k"), fem.cylinder_case("S2k").dof_xy()):  # (the examples' coordinates are the reference's)
        assert np.array_equal(mine, theirs)
    assert np.allclose(ref.dense_gains("S2k", 0.2, 0.0)[:2], np.array(ref.GAINS_REAL_SHIFT), rtol=0.0, atol=1e-6)


def test_weighted_is_scipys_product_bit_for_bit():
    _, M = ref.case("S2k")
    x, y = ref.dof_xy("S2k")
    box, smooth = ref.window("S2k", *ref.OMEGA_F), 0.5 * (1.0 + np.tanh(x - 2.0))
    for left, right in ((box, None), (smooth, None), (smooth, 1.0 + y * y), (np.ones(M.shape[0]), None)):
        r = left if right is None else right
        want = (sp.diags(left) @ M @ sp.diags(r)).toarray()
        assert np.array_equal(ref.weighted(M, left, right).toarray(), want)
    assert np.array_equal(ref.weighted(M, np.ones(M.shape[0])).data, M.data)


@pytest.mark.parametrize("nsteps", [16])
def test_growth_march_with_the_weight_at_the_turn(nsteps):
    """The dense windowed gains are the listed ones, a window of ones gives ``growth_reference.GAINS``, and the restated iteration on
    the march with Q at the turn reaches the dense values to 1e-12 G_1 under Euler; under SDIRK2 its W is M-self-adjoint to rounding."""
    A, M = ref.case("S2k")
    keep = gref.keep_mask("S2k")
    Q = ref.weight_of("S2k", ref.OMEGA_Q)
    dense = ref.dense_growth_gains("S2k", nsteps, ref.OMEGA_Q)[:3]
    assert np.allclose(dense, np.array(ref.GROWTH_GAINS[nsteps]), rtol=0.0, atol=1e-6)
    ones = ref.weighted(M, np.ones(M.shape[0]))
    v0 = gref.start_vector(A.shape[0])
    out = sref.march_trl(ref.TurnedMarch(gref.HostMarch(A, M, gref.DT, keep), Q), nsteps, 3, 12, 1e-10, v0)
    err = np.abs(out["gains"] - dense).max() / dense[0]
    print(f"N = {nsteps}: windowed gains {out['gains']}, |G - dense|_max / G_1 = {err:.2e}, {out['restarts']} restarts")
    assert len(out["gains"]) == 3 and err <= 1e-12
    plain, turned = gref.HostMarch(A, M, gref.DT, keep), ref.TurnedMarch(gref.HostMarch(A, M, gref.DT, keep), ones)
    close = lambda x, y: np.abs(x - y).max() <= 1e-12 * np.abs(y).max()  # noqa: E731  (the stages commute: the same vector up to rounding)
    assert close(turned.W(v0, 3), plain.W(v0, 3))
    sd = ref.TurnedMarch(sref.SdirkMarch(A, M, sref.DT, keep), Q)
    u, v = keep * v0, keep * gref.start_vector(A.shape[0], 1)
    a, b = u @ (M @ sd.W(v, 2)), v @ (M @ sd.W(u, 2))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    sd1 = ref.TurnedMarch(sref.SdirkMarch(A, M, sref.DT, keep), ones)
    assert close(sd1.W(v0, 2), sref.SdirkMarch(A, M, sref.DT, keep).W(v0, 2))


def test_dense_growth_with_ones_is_the_plain_table():
    assert np.allclose(ref.dense_growth_gains("S2k", 16, None)[:3], np.array(gref.GAINS[("S2k", 16)]), rtol=0.0, atol=1e-6)


def _pair():
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0.0], [0.0, 3.0, 1.0], [1.0, 0.0, 4.0]]))
    M = sp.csr_matrix(np.diag([1.0, 1.0, 0.0]))
    return A, M


def _no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the refusals below come before GPU work."""
    import lsa_hip

    def boom(*a, **k):
        raise AssertionError("a device context was opened")

    monkeypatch.setattr(lsa_hip, "Context", boom)


def test_resolvent_front_end_refusals(monkeypatch):
    from Solver.resolvent import ResolventConfig, ResolventSolver

    _no_device(monkeypatch)
    A, M = _pair()
    cfg = ResolventConfig(num_modes=1, ncv=2)
    ok = np.array([1.0, 0.5, 0.0])
    for side in ("forcing", "response"):
        w, q = f"{side}_window", f"{side}_weight"
        with pytest.raises(ValueError, match="not both"):
            ResolventSolver(A, M, cfg, **{w: ok, q: M})
        with pytest.raises(ValueError, match="shape"):
            ResolventSolver(A, M, cfg, **{w: np.ones(4)})
        with pytest.raises(ValueError, match="shape"):
            ResolventSolver(A, M, cfg, **{w: np.ones((3, 1))})
        with pytest.raises(ValueError, match="negative"):
            ResolventSolver(A, M, cfg, **{w: np.array([1.0, -1.0, 0.0])})
        with pytest.raises(ValueError, match="NaN"):
            ResolventSolver(A, M, cfg, **{w: np.array([1.0, np.nan, 0.0])})
        with pytest.raises(ValueError, match="NaN"):
            ResolventSolver(A, M, cfg, **{w: np.array([1.0, np.inf, 0.0])})
        with pytest.raises(ValueError, match="complex"):
            ResolventSolver(A, M, cfg, **{w: np.array([1.0, 1.0j, 0.0])})
        with pytest.raises(ValueError, match="no mass"):
            ResolventSolver(A, M, cfg, **{w: np.array([0.0, 0.0, 1.0])})  # (only the massless dof is inside)
        with pytest.raises(ValueError, match="shape"):
            ResolventSolver(A, M, cfg, **{q: sp.identity(4, format="csr")})
        with pytest.raises(ValueError, match="complex"):
            ResolventSolver(A, M, cfg, **{q: (M * (1.0 + 0.0j)).tocsr()})
        with pytest.raises(ValueError, match="symmetric"):
            ResolventSolver(A, M, cfg, **{q: sp.csr_matrix(np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))})
        with pytest.raises(ValueError, match="NaN"):
            ResolventSolver(A, M, cfg, **{q: sp.csr_matrix(np.diag([1.0, np.nan, 1.0]))})
    for bad in (float("nan"), float("inf"), 0.1j, "x"):
        with pytest.raises(ValueError, match="discount"):
            ResolventSolver(A, M, cfg, discount=bad)
    rs = ResolventSolver(A, M, cfg, forcing_window=ok, response_weight=M, discount=0.1)
    with pytest.raises(ValueError, match="discount"):
        rs.solve(0.4, discount=float("nan"))
    with pytest.raises(ValueError, match="discount"):
        rs.solve(0.4, discount=0.2j)
    with pytest.raises(ValueError, match="real"):
        rs.solve(0.5j)  # (omega stays a real frequency: the discount is the way to a complex shift)
    with pytest.raises(ValueError, match="finite"):
        rs.norm_map([0.1 + 0.2j, complex(np.nan, 0.0)])


def test_growth_front_end_refusals(monkeypatch):
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    _no_device(monkeypatch)
    A, M = _pair()
    cfg = TransientGrowthConfig(dt=0.25, num_modes=1, ncv=2)
    with pytest.raises(ValueError, match="not both"):
        TransientGrowthSolver(A, M, cfg, response_window=np.ones(3), response_weight=M)
    with pytest.raises(ValueError, match="shape"):
        TransientGrowthSolver(A, M, cfg, response_window=np.ones(2))
    with pytest.raises(ValueError, match="negative"):
        TransientGrowthSolver(A, M, cfg, response_window=np.array([1.0, -0.5, 1.0]))
    with pytest.raises(ValueError, match="NaN"):
        TransientGrowthSolver(A, M, cfg, response_window=np.array([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError, match="complex"):
        TransientGrowthSolver(A, M, cfg, response_window=np.array([1.0, 1.0j, 1.0]))
    with pytest.raises(ValueError, match="no mass"):
        TransientGrowthSolver(A, M, cfg, response_window=np.array([0.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="symmetric"):
        TransientGrowthSolver(A, M, cfg, response_weight=sp.csr_matrix(np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])))
    with pytest.raises(ValueError, match="shape"):
        TransientGrowthSolver(A, M, cfg, response_weight=sp.identity(4, format="csr"))
    TransientGrowthSolver(A, M, cfg, response_window=np.array([1.0, 0.0, 0.0]))  # (a valid window is taken without a device)


def test_result_dataclasses_keep_their_positional_order():
    from Solver.growth import TransientGrowthResult
    from Solver.resolvent import ResolventResult

    names = [f.name for f in dataclasses.fields(ResolventResult)]
    assert names == ["omega", "gains", "responses", "forcings", "estimates", "stats", "discount"]
    r = ResolventResult(0.4, np.ones(1), np.ones((2, 1)), None, np.zeros(1), {"a": 1})
    assert r.stats == {"a": 1} and r.discount == 0.0
    names = [f.name for f in dataclasses.fields(TransientGrowthResult)]
    assert names == ["horizon", "steps", "dt", "gains", "initial", "responses", "energy", "times", "estimates", "stats", "scheme", "response_energy"]
    g = TransientGrowthResult(1.0, 4, 0.25, np.ones(1), np.ones((2, 1)), np.ones((2, 1)), np.ones((1, 5)), np.arange(5.0), np.zeros(1), {}, "sdirk2")
    assert g.scheme == "sdirk2" and g.response_energy is None


def test_norm_map_visits_the_real_points_as_one_group(monkeypatch):
    """With the device work stubbed out: the points off the real axis in the order given, then the real ones; the previous point's
    response is the next one's start vector exactly when warm_start is on; the results and statistics return in the order given."""
    from Solver.resolvent import ResolventConfig, ResolventSolver

    _no_device(monkeypatch)
    A, M = _pair()
    rs = ResolventSolver(A, M, ResolventConfig(num_modes=1, ncv=2))
    pts = np.array([[0.2 + 0.0j, 0.1 + 0.4j, -0.3 + 0.0j], [0.1 - 0.4j, 0.5 + 0.0j, -0.05 + 0.7j]])
    assert ResolventSolver.map_order(pts) == [1, 3, 5, 0, 2, 4]
    for warm_start in (True, False):
        seen = []

        def stub(z, warm, seen=seen):
            seen.append((z, None if warm is None else warm.copy()))
            return abs(z) + 1.0, np.full(3, z), {"z": z}

        monkeypatch.setattr(rs, "_gain_at", stub)
        got = rs.norm_map(pts, warm_start=warm_start)
        order = [z for z, _ in seen]
        assert order == [pts.ravel()[i] for i in (1, 3, 5, 0, 2, 4)]
        kinds = [z.imag == 0.0 for z in order]
        assert kinds == sorted(kinds)  # (one switch from complex to real factors: at most two preparations)
        assert got.shape == pts.shape and np.array_equal(got, np.abs(pts) + 1.0)
        assert [s["z"] for s in rs.last_map_stats] == list(pts.ravel())
        assert seen[0][1] is None
        for (z, warm), (zprev, _) in zip(seen[1:], seen[:-1]):
            assert (warm is None) if not warm_start else np.array_equal(warm, np.full(3, zprev))


def test_library_and_binding_carry_the_entries():
    import lsa_hip

    lib = lsa_hip.load_library()
    for name in ("lsa_csr_window", "lsa_resolvent_set_weights", "lsa_growth_set_response_weight", "lsa_growth_response_energy"):
        assert name in lsa_hip.SIGNATURES and hasattr(lib, name)
    assert hasattr(lsa_hip.CsrMatrix, "windowed") and hasattr(lsa_hip.ResolventBasis, "set_weights")
    assert hasattr(lsa_hip.GrowthBasis, "set_response_weight")
