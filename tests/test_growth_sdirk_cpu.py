"""CPU suite of the second-order time stepping of the transient-growth analysis (SDIRK2, ``tests/growth_sdirk_reference.py``): the
numpy restatement of the library's iteration on the two-stage march pinned against the dense optimal gains, the pinned gains, the
order of convergence in dt, and the front end's ``scheme`` field.  The GPU suite (``tests/test_gpu_growth_sdirk.py``) holds the
library to the bounds this restatement meets."""

import numpy as np
import pytest

import helpers  # noqa: F401
import growth_reference as ref
import growth_sdirk_reference as sref


@pytest.mark.parametrize("dt,nsteps,counts", [(0.5, 1, None), (0.5, 2, None), (0.5, 8, (4, 35)), (0.5, 20, (3, 29)), (0.25, 16, (4, 35))])
def test_restatement_against_the_dense_gains(dt, nsteps, counts):
    """S2k, num_modes 3, ncv 12, tol 1e-10, the seeded start vector: the restatement on the SDIRK2 march matches the dense gains to
    1e-12 G_1 (it reaches 3e-14), descending, with the pinned restart and apply counts where the path through the restarts is short
    enough to be stable (N = 1: 10 restarts, 71 applies; N = 2: 9 and 65, when written); its initial conditions are M-orthonormal and
    zero on the constrained rows, and marching them gives the gains back."""
    A, M = ref.case("S2k")
    keep = ref.keep_mask("S2k")
    dense = sref.dense_gains("S2k", dt, nsteps)[:3]
    out = sref.sdirk_trl("S2k", dt, nsteps, 3, 12, 1e-10, ref.start_vector(A.shape[0]))
    err = np.abs(out["gains"] - dense).max() if len(out["gains"]) == 3 else np.inf
    print(f"dt = {dt}, N = {nsteps}: dense {dense}, restatement {out['restarts']} restarts, {out['applies']} applies, |G - dense|_max / G_1 = {err / dense[0]:.2e}")
    assert err <= 1e-12 * dense[0]
    assert (np.diff(out["gains"]) <= 0.0).all()
    if counts is not None:
        assert (out["restarts"], out["applies"]) == counts
    Q0 = out["Q0"]
    host = sref.SdirkMarch(A, M, dt, keep)
    assert np.abs(Q0.T @ (host.M @ Q0) - np.eye(3)).max() <= 1e-10
    assert not Q0[keep == 0.0].any()
    end = np.column_stack([host.march(q, nsteps)[:, -1] for q in Q0.T])
    assert np.abs(host.energy(end) - out["gains"]).max() <= 1e-8 * dense[0]


@pytest.mark.parametrize("dt,nsteps", sorted(sref.GAINS))
def test_pinned_gains(dt, nsteps):
    """The dense SDIRK2 gains of S2k are the listed six-decimal ones."""
    dense = sref.dense_gains("S2k", dt, nsteps)[:3]
    print(f"dt = {dt}, N = {nsteps}: dense {dense}")
    assert np.allclose(dense, np.array(sref.GAINS[(dt, nsteps)]), rtol=0.0, atol=1e-6)


def test_second_order_in_dt():
    """T = 4 at dt = 0.5, 0.25, 0.125: (G(0.5) - G(0.25)) / (G(0.25) - G(0.125)) lies in [3.5, 4.7] for G_1 and G_2 (a second-order
    scheme in its asymptotic range gives 4; it was 4.19 for both), and below 2 for implicit Euler on the same three steps."""
    ratios = {}
    for scheme in ("sdirk2", "euler"):
        g = [sref.dense_gains("S2k", dt, round(4.0 / dt), scheme)[:2] for dt in (0.5, 0.25, 0.125)]
        ratios[scheme] = (g[0] - g[1]) / (g[1] - g[2])
        print(f"{scheme}: G(T = 4) at dt = 0.5, 0.25, 0.125: {g}; ratios {ratios[scheme]}")
    assert ((ratios["sdirk2"] >= 3.5) & (ratios["sdirk2"] <= 4.7)).all()
    assert (ratios["euler"] < 2.0).all()
    assert np.allclose(sref.dense_gains("S2k", 0.25, 16, "euler")[:3], np.array(ref.GAINS[("S2k", 16)]), rtol=0.0, atol=1e-6)


def test_the_two_stage_step_is_the_stability_function():
    """On the scalar pair M = 1, A = lambda the host step multiplies by (1 + (1 - 2 gamma) z) / (1 - gamma z)^2, z = lambda dt."""
    import scipy.sparse as sp

    for lam in (-0.3, -7.0, -4000.0):
        host = sref.SdirkMarch(sp.csr_matrix([[lam]]), sp.csr_matrix([[1.0]]), 0.5)
        z, g = lam * 0.5, sref.GAMMA
        assert host.step(np.array([1.0]))[0] == pytest.approx((1.0 + (1.0 - 2.0 * g) * z) / (1.0 - g * z) ** 2, rel=1e-13)
        assert host.step(np.array([1.0]), "T")[0] == pytest.approx(host.step(np.array([1.0]))[0], rel=1e-15)


def test_scheme_field_of_the_front_end():
    """``scheme`` is the config's last field and defaults to implicit Euler; an unknown one is a ValueError before any device work
    (there is no device here); ``sdirk2`` sets the shift to 1 / (gamma dt) and leaves the horizons whole multiples of dt."""
    import dataclasses

    import scipy.sparse as sp

    from Solver.growth import TransientGrowthConfig, TransientGrowthResult, TransientGrowthSolver

    assert TransientGrowthConfig(dt=0.5).scheme == "euler"
    assert [f.name for f in dataclasses.fields(TransientGrowthConfig)][-1] == "scheme"
    assert TransientGrowthConfig(dt=0.5) == TransientGrowthConfig(dt=0.5, num_modes=1, ncv=12, atol=1e-8, max_it=500, scheme="euler")
    with pytest.raises(ValueError, match="scheme"):
        TransientGrowthConfig(dt=0.5, scheme="rk4")
    assert "scheme" in [f.name for f in dataclasses.fields(TransientGrowthResult)]
    A = sp.csr_matrix(np.array([[-2.0, 1.0, 0.0], [0.0, -3.0, 1.0], [1.0, 0.0, -4.0]]))
    M = sp.identity(3, format="csr")
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(dt=0.5, num_modes=1, ncv=2, scheme="sdirk2"))
    assert tg.config.scheme == "sdirk2"
    assert tg.solver._target == complex(1.0 / ((1.0 - 1.0 / np.sqrt(2.0)) * 0.5))
    assert TransientGrowthSolver(A, M, TransientGrowthConfig(dt=0.5, num_modes=1, ncv=2)).solver._target == complex(2.0)
    with pytest.raises(ValueError, match="multiple"):
        tg.solve(0.75)


def test_library_and_binding_carry_the_entry():
    import lsa_hip

    lib = lsa_hip.load_library()
    assert "lsa_growth_set_scheme" in lsa_hip.SIGNATURES and hasattr(lib, "lsa_growth_set_scheme")
    assert lsa_hip.GrowthBasis.SCHEMES == {"euler": 0, "sdirk2": 1}
