"""CPU suite of the transient-growth analysis: the numpy restatement of the library's masked iteration (``tests/growth_reference.py``)
pinned against the dense optimal gains, the front end's rule for constrained dofs and its argument errors, and the presence of the
C-ABI entries.  The GPU suite (``tests/test_gpu_growth.py``) holds the library to the bounds this restatement meets."""

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import growth_reference as ref


@pytest.mark.parametrize("case,nsteps,nev,ncv,counts", [("S2k", 16, 3, 12, (4, 35)), ("S2k", 40, 3, 12, None), ("S2k", 80, 2, 12, None),
                                                         ("S5k", 16, 4, 16, (2, 32))])
def test_restatement_against_the_dense_gains(case, nsteps, nev, ncv, counts):
    """dt = 0.25, tol 1e-10, the seeded start vector.  The dense gains (squared singular values of M^(1/2) Xi M^(1/2) on the free dofs)
    are the listed six-decimal ones; the restatement matches them to 1e-10 G_1 (the bound of the GPU suite; it reaches 5e-15), with
    the pinned restart and apply counts where the path through the restarts is short enough to be stable, its initial conditions are
    M-orthonormal and exactly zero on the constrained rows, and marching them gives the gains back."""
    A, M = ref.case(case)
    keep = ref.keep_mask(case)
    expected = np.array(ref.GAINS[(case, nsteps)])
    dense = ref.dense_gains(case, nsteps)[:nev]
    assert np.allclose(dense, expected, rtol=0.0, atol=1e-6)
    out = ref.growth_trl(A, M, ref.DT, nsteps, keep, nev, ncv, 1e-10, ref.start_vector(A.shape[0]))
    err = np.abs(out["gains"] - dense).max() if len(out["gains"]) == nev else np.inf
    print(f"{case} N = {nsteps}: dense {dense}, restatement {out['restarts']} restarts, {out['applies']} applies, |G - dense|_max / G_1 = {err / dense[0]:.2e}")
    assert err <= 1e-10 * dense[0]
    assert (np.diff(out["gains"]) <= 0.0).all()
    if counts is not None:
        assert (out["restarts"], out["applies"]) == counts
    Q0 = out["Q0"]
    host = ref.HostMarch(A, M, ref.DT, keep)
    assert np.abs(Q0.T @ (host.M @ Q0) - np.eye(nev)).max() <= 1e-10
    assert not Q0[keep == 0.0].any()
    end = np.column_stack([host.march(q, nsteps)[:, -1] for q in Q0.T])
    assert np.abs(host.energy(end) - out["gains"]).max() <= 1e-8 * dense[0]
    for q in Q0.T:
        assert q[int(np.argmax(np.abs(q)))] > 0.0


def test_the_mask_matters():
    """Unmasked, S2k at N = 16 has the 44-fold spurious gain (1 - dt)^(-2 N) = 0.75^-32 of its identity rows."""
    A, M = ref.case("S2k")
    out = ref.growth_trl(A, M, ref.DT, 16, None, 1, 12, 1e-10, ref.start_vector(A.shape[0]))
    assert abs(out["gains"][0] - ref.SPURIOUS_S2K_N16) <= 1e-8 * ref.SPURIOUS_S2K_N16
    assert abs(ref.SPURIOUS_S2K_N16 - 9954.961195) <= 1e-5


@pytest.mark.parametrize("case", ["S2k", "S5k"])
def test_auto_rule_finds_the_identity_rows(case):
    """constrained="auto": exactly the rows that are identity rows in both A and M (44 of 1953, 71 of 4851); a coupled index is refused,
    a decoupled one accepted, None masks nothing."""
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver, decoupled_dofs

    A, M = ref.case(case)
    cfg = TransientGrowthConfig(dt=ref.DT)
    tg = TransientGrowthSolver(A, M, cfg)
    found = tg.constrained
    assert found.size == ref.CONSTRAINED[case]
    assert np.array_equal(found, ref.decoupled_rows(A, M)) and np.array_equal(found, decoupled_dofs(A, M))
    eye = sp.identity(A.shape[0], format="csr")
    identity_rows = np.flatnonzero((abs(A - eye).sum(axis=1).A1 == 0.0) & (abs(M - eye).sum(axis=1).A1 == 0.0))
    assert np.array_equal(found, identity_rows)
    coupled = int(np.setdiff1d(np.arange(A.shape[0]), found)[0])
    with pytest.raises(ValueError, match="coupled"):
        TransientGrowthSolver(A, M, cfg, constrained=[int(found[0]), coupled])
    with pytest.raises(ValueError, match="outside"):
        TransientGrowthSolver(A, M, cfg, constrained=[A.shape[0]])
    assert np.array_equal(TransientGrowthSolver(A, M, cfg, constrained=found[:3]).constrained, found[:3])
    assert TransientGrowthSolver(A, M, cfg, constrained=None).constrained.size == 0


def _pair():
    A = sp.csr_matrix(np.array([[-2.0, 1.0, 0.0], [0.0, -3.0, 1.0], [1.0, 0.0, -4.0]]))
    M = sp.identity(3, format="csr")
    return A, M


def test_front_end_argument_errors():
    """What the front end refuses before any device work (there is no device here)."""
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver, horizon_steps
    from Solver.utils import PreconditionerType

    A, M = _pair()
    cfg = TransientGrowthConfig(dt=0.25, num_modes=1, ncv=2)
    crooked = sp.csr_matrix(np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="symmetric"):
        TransientGrowthSolver(A, crooked, cfg)
    with pytest.raises(ValueError, match="M is complex"):
        TransientGrowthSolver(A, (M * (1.0 + 0.0j)).tocsr(), cfg)
    with pytest.raises(ValueError, match="A is complex"):
        TransientGrowthSolver((A * (1.0 + 0.0j)).tocsr(), M, cfg)
    with pytest.raises(ValueError, match="needs M"):
        TransientGrowthSolver(A, None, cfg)
    for dt in (0.0, -0.25, float("nan")):
        with pytest.raises(ValueError, match="dt"):
            TransientGrowthSolver(A, M, TransientGrowthConfig(dt=dt))
    with pytest.raises(ValueError, match="ncv"):
        TransientGrowthSolver(A, M, TransientGrowthConfig(dt=0.25, num_modes=3, ncv=3))
    with pytest.raises(ValueError, match="constrained"):
        TransientGrowthSolver(A, M, cfg, constrained="all")
    with pytest.raises(NotImplementedError, match="layout"):
        TransientGrowthSolver(A, M, cfg, layout="sharded")
    with pytest.raises(NotImplementedError, match="exact LU"):
        TransientGrowthSolver(A, M, cfg, pc_type=PreconditionerType.ILU)
    tg = TransientGrowthSolver(A, M, cfg)
    for T in (0.0, -1.0, 0.1, 0.3, 1.0 + 1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="multiple"):
            tg.solve(T)
    with pytest.raises(ValueError, match="multiple"):
        tg.sweep([1.0, 0.3])
    assert horizon_steps(4.0, 0.25) == 16 and horizon_steps(0.25, 0.25) == 1 and horizon_steps(3 * 0.1, 0.1) == 3
    assert horizon_steps(4.0 * (1.0 + 5e-10), 0.25) == 16
    assert tg.config.num_modes == 1 and TransientGrowthConfig(dt=0.5) == TransientGrowthConfig(dt=0.5, num_modes=1, ncv=12, atol=1e-8, max_it=500)


def test_library_and_binding_carry_the_entries():
    import lsa_hip

    lib = lsa_hip.load_library()
    for name in ("lsa_growth_create", "lsa_growth_destroy", "lsa_growth_set_row_permutation", "lsa_growth_set_steps", "lsa_growth_set_start",
                 "lsa_growth_extend", "lsa_growth_basis", "lsa_growth_solve"):
        assert name in lsa_hip.SIGNATURES and hasattr(lib, name)
    assert hasattr(lsa_hip, "GrowthBasis")
