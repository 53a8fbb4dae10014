"""GPU suite: transient growth (``csrc/growth.hip``, ``lsa_growth_solve``, ``Solver.growth``) on the synthetic cylinder cases S2k
(n = 1953: no multiple of 256 or 512, the last chunk of every reduction is partial; 44 constrained rows) and S5k (n = 4851; 71), at
dt = 0.25, against dense gains and a SuperLU march on the host.  The bounds are those of the resolvent and the symmetric path's suites
(``test_gpu_resolvent.py``, ``test_gpu_lanczos.py``) for the same kind of quantity and of the numpy restatement in
``tests/growth_reference.py``, which ``test_growth_cpu.py`` pins."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import helpers  # noqa: F401
import growth_reference as ref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


def run_child(job, case, ncv, nsteps, out, **env):
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, str(HERE / "growth_child.py"), job, case, str(ncv), str(nsteps), str(out)], check=True, env=e, timeout=600)
    return np.load(out)


@pytest.mark.parametrize("nsteps", [1, 2, 3])
def test_basis_and_lanczos_relation(hip_ctx, nsteps):
    """Twelve steps through lsa_growth_extend on S2k for N = 1 (the single marched solve), 2 and 3 (both parities of the march's
    alternating right-hand sides): T symmetric tridiagonal with positive off-diagonals, ||V^T M V - I||_max <= 1e-12, the M-norm defect
    of W V_m - V_{m+1} T <= 1e-10 ||T||_F with W applied by the SuperLU march, and the rows of V on masked indices exactly 0.0.  The
    injection and the steps pass ncols = 0, 1, ..., 12 through the tiles."""
    import lsa_hip

    A0, M0 = ref.case("S2k")
    A, M = on_shared_pattern(A0, M0)
    n, m = A.shape[0], 12
    keep = ref.keep_mask("S2k")
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, 1.0 / ref.DT, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.GrowthBasis(hip_ctx, op, m, nsteps, keep)
    basis.set_start(ref.start_vector(n))
    Tfull = np.zeros((m + 1, m), order="F")
    assert basis.extend(0, m, Tfull) == -1
    V = basis.basis(m + 1)
    st = op.stats()
    del basis, op
    T = Tfull[:m, :m]
    assert np.array_equal(T, T.T) and np.count_nonzero(np.triu(T, 2)) == 0
    assert (np.diag(Tfull, -1) > 0.0).all()
    host = ref.HostMarch(A0, M0, ref.DT, keep)
    orth = np.abs(V.T @ (host.M @ V) - np.eye(m + 1)).max()
    D = np.column_stack([host.W(V[:, j], nsteps) for j in range(m)]) - V @ Tfull
    defect, tn = float(np.sqrt(np.clip(host.energy(D), 0.0, None).sum())), np.linalg.norm(Tfull)
    print(f"N = {nsteps}: |V^T M V - I|_max = {orth:.2e}; relation defect / |T|_F = {defect / tn:.2e}; refined solves {st['refined_solves']}")
    assert orth <= 1e-12
    assert defect <= 1e-10 * tn
    assert (V[keep == 0.0] == 0.0).all()


@pytest.mark.parametrize("case,ncv,nsteps", [("S2k", 12, 3), ("S5k", 20, 2)])
def test_fused_march_against_the_unfused_form(tmp_path, case, ncv, nsteps):
    """The same steps in two child processes, tg_march_kernel + tg_log_kernel and LSA_GROWTH_FUSED=0 (k_residual_norms, k_multi_dot, the
    scale): T and V byte for byte alike."""
    fused = run_child("basis", case, ncv, nsteps, tmp_path / "fused.npz")
    plain = run_child("basis", case, ncv, nsteps, tmp_path / "plain.npz", LSA_GROWTH_FUSED="0")
    assert int(fused["bd"]) == -1 and int(plain["bd"]) == -1
    dT, dV = np.abs(plain["T"] - fused["T"]).max(), np.abs(plain["V"] - fused["V"]).max()
    print(f"{case}: fused against unfused: |dT|_max = {dT:.2e}, |dV|_max = {dV:.2e}")
    assert np.array_equal(fused["T"], plain["T"])
    assert np.array_equal(fused["V"], plain["V"])


CFG = dict(dt=ref.DT, num_modes=3, ncv=12, atol=1e-10)
_SOLVED = {}


def fresh(nsteps, **kw):
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case("S2k")
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(**{**CFG, **kw.pop("cfg", {})}), **kw)
    res = tg.solve(nsteps * ref.DT)
    tg.release()
    return res


def solved(nsteps):
    """One front-end solve per horizon and process: S2k, num_modes 3, ncv 12, atol 1e-10."""
    if nsteps not in _SOLVED:
        _SOLVED[nsteps] = fresh(nsteps)
    return _SOLVED[nsteps]


@pytest.mark.parametrize("nsteps", [16, 40])
def test_gains_against_dense(nsteps):
    """|G_i - G_i^dense| <= 1e-10 G_1 (the numpy restatement reaches 5e-15), the gains descending, at least one restart (the restatement:
    4 at N = 16), and at least N solves of each direction per application of W."""
    res = solved(nsteps)
    dense = ref.dense_gains("S2k", nsteps)[:3]
    err = np.abs(res.gains - dense).max() if len(res.gains) == 3 else np.inf
    print(f"N = {nsteps}: gains {res.gains}, |G - dense|_max / G_1 = {err / dense[0]:.2e}, stats {res.stats}")
    assert res.steps == nsteps and res.horizon == nsteps * ref.DT and res.dt == ref.DT
    assert np.allclose(dense, np.array(ref.GAINS[("S2k", nsteps)]), rtol=0.0, atol=1e-6)
    assert len(res.gains) == 3 and (np.diff(res.gains) <= 0.0).all()
    assert err <= 1e-10 * dense[0]
    assert res.stats["restarts"] >= 1
    assert res.stats["forward_solves"] >= nsteps * res.stats["applies"] and res.stats["transposed_solves"] >= nsteps * res.stats["applies"]


def test_pairs_and_energy():
    """The N = 16 solve: ||Q0^T M Q0 - I||_max <= 1e-10, energy[i, 0] = 1 to 1e-12, energy[i, N] = G_i and ||responses_i||_M^2 = G_i to
    1e-10 relative, the whole energy curve within 1e-8 relative of a SuperLU march from the returned initial[:, i], initial exactly zero
    on the 44 masked rows and the largest entry of each column positive."""
    res = solved(16)
    A, M = ref.case("S2k")
    keep = ref.keep_mask("S2k")
    host = ref.HostMarch(A, M, ref.DT, keep)
    Q0, QT, E = res.initial, res.responses, res.energy
    assert Q0.shape == (A.shape[0], 3) and QT.shape == Q0.shape and E.shape == (3, 17) and np.array_equal(res.times, ref.DT * np.arange(17))
    orth = np.abs(Q0.T @ (host.M @ Q0) - np.eye(3)).max()
    e_resp = host.energy(QT)
    curves = np.array([host.energy(host.march(Q0[:, i], 16)) for i in range(3)])
    print(f"|Q0^T M Q0 - I|_max = {orth:.2e}, |E_0 - 1|_max = {np.abs(E[:, 0] - 1.0).max():.2e}, |E_N / G - 1|_max = "
          f"{np.abs(E[:, 16] / res.gains - 1.0).max():.2e}, | |resp|_M^2 / G - 1|_max = {np.abs(e_resp / res.gains - 1.0).max():.2e}, "
          f"|E / march - 1|_max = {np.abs(E / curves - 1.0).max():.2e}")
    assert orth <= 1e-10
    assert np.abs(E[:, 0] - 1.0).max() <= 1e-12
    assert np.abs(E[:, 16] - res.gains).max() <= 1e-10 * res.gains.min() and (np.abs(E[:, 16] / res.gains - 1.0) <= 1e-10).all()
    assert (np.abs(e_resp / res.gains - 1.0) <= 1e-10).all()
    assert (np.abs(E / curves - 1.0) <= 1e-8).all()
    assert (keep == 0.0).sum() == 44 and (Q0[keep == 0.0] == 0.0).all()
    for q in Q0.T:
        assert q[int(np.argmax(np.abs(q)))] > 0.0


def test_the_mask_matters():
    """S2k, constrained=None, one mode, N = 16: the gain is the spurious boundary mode's 0.75^-32 = 9954.961195... to 1e-8 relative --
    what the default mask removes."""
    res = fresh(16, constrained=None, cfg=dict(num_modes=1))
    print(f"unmasked gain {res.gains}, 0.75^-32 = {ref.SPURIOUS_S2K_N16!r}")
    assert len(res.gains) == 1 and abs(res.gains[0] / ref.SPURIOUS_S2K_N16 - 1.0) <= 1e-8
    assert res.stats["constrained"] == 0


def test_sweep_on_one_factorisation():
    """sweep([2, 4, 10]) on one solver: the second and third horizon on the first one's factorisation (the operator's factor clock
    does not move), gains, initial conditions and energies byte for byte those of three fresh solvers."""
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case("S2k")
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(**CFG))
    swept = tg.sweep([2.0, 4.0, 10.0])
    tg.release()
    assert [r.steps for r in swept] == [8, 16, 40]
    assert not swept[0].stats["factorisation_reused"] and swept[1].stats["factorisation_reused"] and swept[2].stats["factorisation_reused"]
    assert swept[1].stats["seconds_factor"] == swept[0].stats["seconds_factor"] == swept[2].stats["seconds_factor"]
    for got in swept:
        one = solved(got.steps)
        for key in ("gains", "initial", "energy"):
            assert np.array_equal(getattr(got, key), getattr(one, key)), (got.steps, key)


def test_two_processes_give_the_same_bytes(tmp_path):
    """S5k, N = 16, num_modes 4, ncv 16 in two fresh processes: every output byte for byte alike, the gains the dense ones to 1e-5."""
    a = run_child("solve", "S5k", 16, 16, tmp_path / "a.npz")
    b = run_child("solve", "S5k", 16, 16, tmp_path / "b.npz")
    print(f"S5k gains {a['gains']}, restarts {int(a['restarts'])}")
    for key in ("gains", "initial", "responses", "energy", "estimates"):
        assert np.array_equal(a[key], b[key]), key
    assert np.allclose(a["gains"], np.array(ref.GAINS[("S5k", 16)]), rtol=0.0, atol=1e-5)


def test_create_refuses_what_it_cannot_run(hip_ctx):
    """lsa_growth_create: LSA_ERR_ARG with a message that names the condition for an operator in adjoint mode, a projected one, one
    without M, one with an ILU, one at a complex shift, and for nsteps = 0; it takes the operator once adjoint and projection are
    undone."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    n = A.shape[0]
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    sigma = 1.0 / ref.DT

    def refused(op, word, nsteps=4):
        with pytest.raises(ValueError) as info:  # (how the binding reports LSA_ERR_ARG; every other status is an LsaError)
            lsa_hip.GrowthBasis(hip_ctx, op, 12, nsteps)
        assert not isinstance(info.value, lsa_hip.LsaError) and "lsa_growth_create" in str(info.value) and word in str(info.value), str(info.value)

    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, sigma, mode=0, pc_type=2, ksp_rtol=1e-12)
    op.set_adjoint(True)
    refused(op, "adjoint")
    op.set_adjoint(False)
    keep = np.ones(n)
    keep[::7] = 0.0
    op.set_projection(keep)
    refused(op, "projected")
    op.set_projection(None)
    refused(op, "nsteps", nsteps=0)
    lsa_hip.GrowthBasis(hip_ctx, op, 12, 4)  # (and takes it once both are undone)
    del op
    refused(lsa_hip.ShiftInvertOperator(hip_ctx, dA, None, sigma, mode=0, pc_type=2, ksp_rtol=1e-12), "no M")
    refused(lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, sigma + 0.5j, mode=0, pc_type=2, ksp_rtol=1e-12), "complex")
    # an ILU needs the ordering the front end gives it (in the natural one the pressure row 2 is a zero pivot)
    from Solver.utils import _combine, _permute, pivot_safe_rcm

    perm = pivot_safe_rcm(_combine(A, M, sigma))
    dAp, dMp = lsa_hip.CsrMatrix.from_scipy(hip_ctx, _permute(A, perm)), lsa_hip.CsrMatrix.from_scipy(hip_ctx, _permute(M, perm))
    refused(lsa_hip.ShiftInvertOperator(hip_ctx, dAp, dMp, sigma, mode=0, pc_type=1, ilu_levels=2, ksp_rtol=1e-10), "exact LU")
