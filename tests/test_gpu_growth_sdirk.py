"""GPU suite: transient growth under the second-order SDIRK2 time stepping (``lsa_growth_set_scheme``, the combining form of
``tg_march_kernel``, ``Solver.growth`` with ``scheme="sdirk2"``) on the synthetic cylinder cases S2k (n = 1953: the last chunk of every
reduction is partial; 44 constrained rows) and S5k (n = 4851), at dt = 0.5, against the dense gains and the SuperLU two-stage march of
``tests/growth_sdirk_reference.py``, which ``test_growth_sdirk_cpu.py`` pins.  The bounds are those of ``test_gpu_growth.py`` for the
same quantities."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import helpers  # noqa: F401
import growth_reference as ref
import growth_sdirk_reference as sref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
SIGMA = 1.0 / (sref.GAMMA * sref.DT)


def run_child(case, ncv, nsteps, out, **env):
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, str(HERE / "growth_sdirk_child.py"), case, str(ncv), str(nsteps), str(out)], check=True, env=e, timeout=600)
    return np.load(out)


def twelve_steps(hip_ctx, nsteps, **kw):
    """Twelve steps through lsa_growth_extend on S2k from the seeded start: (T, V, stats of the operator)."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    m = 12
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, kw.pop("sigma", SIGMA), mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.GrowthBasis(hip_ctx, op, m, nsteps, ref.keep_mask("S2k"), **kw)
    basis.set_start(ref.start_vector(A.shape[0]))
    Tfull = np.zeros((m + 1, m), order="F")
    assert basis.extend(0, m, Tfull) == -1
    V = basis.basis(m + 1)
    st, scheme = op.stats(), basis.scheme
    del basis, op
    return Tfull, V, st, scheme


@pytest.mark.parametrize("nsteps", [1, 2, 3])
def test_basis_and_lanczos_relation(hip_ctx, nsteps):
    """Twelve steps through lsa_growth_extend on S2k for N = 1 (four solves: the shortest march with every kind of transition), 2 and 3
    (both parities of the march's alternating right-hand sides): T symmetric tridiagonal with positive off-diagonals,
    ||V^T M V - I||_max <= 1e-12, the M-norm defect of W V_m - V_{m+1} T <= 1e-10 ||T||_F with W applied by the SuperLU two-stage march,
    and the rows of V on masked indices exactly 0.0."""
    m = 12
    Tfull, V, st, scheme = twelve_steps(hip_ctx, nsteps, scheme="sdirk2")
    assert scheme == "sdirk2"
    A0, M0 = ref.case("S2k")
    keep = ref.keep_mask("S2k")
    T = Tfull[:m, :m]
    assert np.array_equal(T, T.T) and np.count_nonzero(np.triu(T, 2)) == 0
    assert (np.diag(Tfull, -1) > 0.0).all()
    host = sref.SdirkMarch(A0, M0, sref.DT, keep)
    orth = np.abs(V.T @ (host.M @ V) - np.eye(m + 1)).max()
    D = np.column_stack([host.W(V[:, j], nsteps) for j in range(m)]) - V @ Tfull
    defect, tn = float(np.sqrt(np.clip(host.energy(D), 0.0, None).sum())), np.linalg.norm(Tfull)
    print(f"N = {nsteps}: |V^T M V - I|_max = {orth:.2e}; relation defect / |T|_F = {defect / tn:.2e}; refined solves {st['refined_solves']}")
    assert orth <= 1e-12
    assert defect <= 1e-10 * tn
    assert (V[keep == 0.0] == 0.0).all()


@pytest.mark.parametrize("case,ncv,nsteps", [("S2k", 12, 3), ("S5k", 20, 2)])
def test_fused_march_against_the_unfused_form(tmp_path, case, ncv, nsteps):
    """The same SDIRK2 steps in two child processes, both forms of tg_march_kernel + tg_log_kernel and LSA_GROWTH_FUSED=0
    (k_residual_norms, k_multi_dot, the scale and the combining pass): T and V byte for byte alike."""
    fused = run_child(case, ncv, nsteps, tmp_path / "fused.npz")
    plain = run_child(case, ncv, nsteps, tmp_path / "plain.npz", LSA_GROWTH_FUSED="0")
    assert int(fused["bd"]) == -1 and int(plain["bd"]) == -1
    dT, dV = np.abs(plain["T"] - fused["T"]).max(), np.abs(plain["V"] - fused["V"]).max()
    print(f"{case}: fused against unfused: |dT|_max = {dT:.2e}, |dV|_max = {dV:.2e}")
    assert np.array_equal(fused["T"], plain["T"])
    assert np.array_equal(fused["V"], plain["V"])


CFG = dict(dt=sref.DT, num_modes=3, ncv=12, atol=1e-10, scheme="sdirk2")
_SOLVED = {}


def fresh(nsteps):
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case("S2k")
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(**CFG))
    res = tg.solve(nsteps * sref.DT)
    tg.release()
    return res


def solved(nsteps):
    """One front-end solve per horizon and process: S2k, dt 0.5, num_modes 3, ncv 12, atol 1e-10, SDIRK2."""
    if nsteps not in _SOLVED:
        _SOLVED[nsteps] = fresh(nsteps)
    return _SOLVED[nsteps]


@pytest.mark.parametrize("nsteps", [8, 20])
def test_gains_against_dense(nsteps):
    """|G_i - G_i^dense| <= 1e-10 G_1 (the numpy restatement reaches 3e-14), the gains descending, at least one restart (the
    restatement: 4 at N = 8, 3 at N = 20), and at least 2 N solves of each direction per application of W."""
    res = solved(nsteps)
    dense = sref.dense_gains("S2k", sref.DT, nsteps)[:3]
    err = np.abs(res.gains - dense).max() if len(res.gains) == 3 else np.inf
    print(f"N = {nsteps}: gains {res.gains}, |G - dense|_max / G_1 = {err / dense[0]:.2e}, stats {res.stats}")
    assert res.scheme == "sdirk2"
    assert res.steps == nsteps and res.horizon == nsteps * sref.DT and res.dt == sref.DT
    assert np.allclose(dense, np.array(sref.GAINS[(sref.DT, nsteps)]), rtol=0.0, atol=1e-6)
    assert len(res.gains) == 3 and (np.diff(res.gains) <= 0.0).all()
    assert err <= 1e-10 * dense[0]
    assert res.stats["restarts"] >= 1
    assert res.stats["forward_solves"] >= 2 * nsteps * res.stats["applies"]
    assert res.stats["transposed_solves"] >= 2 * nsteps * res.stats["applies"]


def test_pairs_and_energy():
    """The N = 8 solve: ||Q0^T M Q0 - I||_max <= 1e-10, energy[i, 0] = 1 to 1e-12, energy[i, N] = G_i and ||responses_i||_M^2 = G_i to
    1e-10 relative, the whole energy curve (time steps, not stages) within 1e-8 relative of a SuperLU two-stage march from the returned
    initial[:, i], initial exactly zero on the 44 masked rows."""
    N = 8
    res = solved(N)
    A, M = ref.case("S2k")
    keep = ref.keep_mask("S2k")
    host = sref.SdirkMarch(A, M, sref.DT, keep)
    Q0, QT, E = res.initial, res.responses, res.energy
    assert Q0.shape == (A.shape[0], 3) and QT.shape == Q0.shape and E.shape == (3, N + 1) and np.array_equal(res.times, sref.DT * np.arange(N + 1))
    orth = np.abs(Q0.T @ (host.M @ Q0) - np.eye(3)).max()
    e_resp = host.energy(QT)
    curves = np.array([host.energy(host.march(Q0[:, i], N)) for i in range(3)])
    print(f"|Q0^T M Q0 - I|_max = {orth:.2e}, |E_0 - 1|_max = {np.abs(E[:, 0] - 1.0).max():.2e}, |E_N / G - 1|_max = "
          f"{np.abs(E[:, N] / res.gains - 1.0).max():.2e}, | |resp|_M^2 / G - 1|_max = {np.abs(e_resp / res.gains - 1.0).max():.2e}, "
          f"|E / march - 1|_max = {np.abs(E / curves - 1.0).max():.2e}")
    assert orth <= 1e-10
    assert np.abs(E[:, 0] - 1.0).max() <= 1e-12
    assert (np.abs(E[:, N] / res.gains - 1.0) <= 1e-10).all()
    assert (np.abs(e_resp / res.gains - 1.0) <= 1e-10).all()
    assert (np.abs(E / curves - 1.0) <= 1e-8).all()
    assert (keep == 0.0).sum() == 44 and (Q0[keep == 0.0] == 0.0).all()


def test_sweep_on_one_factorisation():
    """sweep([2, 4]) on one solver: the second horizon on the first one's factorisation, gains, initial conditions, responses and
    energies byte for byte those of two fresh solvers."""
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case("S2k")
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(**CFG))
    swept = tg.sweep([2.0, 4.0])
    tg.release()
    assert [r.steps for r in swept] == [4, 8] and all(r.scheme == "sdirk2" for r in swept)
    assert not swept[0].stats["factorisation_reused"] and swept[1].stats["factorisation_reused"]
    for got in swept:
        one = solved(got.steps)
        for key in ("gains", "initial", "responses", "energy"):
            assert np.array_equal(getattr(got, key), getattr(one, key)), (got.steps, key)


def test_default_scheme_is_implicit_euler(hip_ctx):
    """GrowthBasis(..., scheme="euler") and the constructor without the argument: the same T and V bytes (N = 3, sigma = 1 / 0.25)."""
    T0, V0, _, s0 = twelve_steps(hip_ctx, 3, sigma=1.0 / ref.DT)
    T1, V1, _, s1 = twelve_steps(hip_ctx, 3, sigma=1.0 / ref.DT, scheme="euler")
    assert s0 == "euler" and s1 == "euler"
    assert np.array_equal(T0, T1) and np.array_equal(V0, V1)


def test_set_scheme_refuses_an_unknown_code(hip_ctx):
    """lsa_growth_set_scheme with code 7: LSA_ERR_ARG, the binding's ValueError naming the scheme; the handle keeps its scheme."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, SIGMA, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.GrowthBasis(hip_ctx, op, 12, 2, scheme="sdirk2")
    with pytest.raises(ValueError) as info:  # (how the binding reports LSA_ERR_ARG; every other status is an LsaError)
        basis.set_scheme_code(7)
    assert not isinstance(info.value, lsa_hip.LsaError) and "lsa_growth_set_scheme" in str(info.value) and "scheme" in str(info.value)
    assert basis.scheme == "sdirk2"
    with pytest.raises(ValueError, match="scheme"):
        lsa_hip.GrowthBasis(hip_ctx, op, 12, 2, scheme="rk4")
    del basis, op
