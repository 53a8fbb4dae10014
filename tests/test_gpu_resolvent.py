"""GPU suite: resolvent analysis (``csrc/resolvent.hip``, ``lsa_resolvent_solve``, ``Solver.resolvent``) on the synthetic cylinder
cases S2k (n = 1953: no multiple of 256 or 512, the last chunk of every reduction is partial) and S5k, against dense gains and
SuperLU on the host.  The bounds are those of the symmetric path's suite (``test_gpu_lanczos.py``) and of the numpy restatement in
``tests/resolvent_reference.py``, which ``test_resolvent_cpu.py`` pins."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import helpers  # noqa: F401
import resolvent_reference as ref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


def run_child(job, case, ncv, out, **env):
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, str(HERE / "resolvent_child.py"), job, case, str(ncv), str(out)], check=True, env=e, timeout=600)
    return np.load(out)


def basis_checks(case, Tfull, V, m):
    """(|V^H M V - I|_max, the M-norm Frobenius defect of W V_m - V_{m+1} T, ||T||_F), W applied by SuperLU."""
    A, M = ref.case(case)
    host = ref.HostResolvent(A, M, ref.OMEGA_TARGET)
    G = V.conj().T @ (M @ V)
    D = np.column_stack([host.W(V[:, j]) for j in range(m)]) - V @ Tfull
    return np.abs(G - np.eye(m + 1)).max(), float(np.sqrt((ref.m_norm_columns(M, D) ** 2).sum())), np.linalg.norm(Tfull)


def test_basis_and_lanczos_relation(hip_ctx):
    """Twelve steps through lsa_resolvent_extend on S2k at the target frequency: T real symmetric tridiagonal with positive
    off-diagonals, ||V^H M V - I||_max <= 1e-12 and the M-norm defect of W V_m - V_{m+1} T <= 1e-10 ||T||_F (the numpy restatement
    reaches 4e-16 and 1.4e-15).  The injection and the steps pass ncols = 0, 1, ..., 12 through the kernels: the empty basis, one
    column, a full column tile of eight (with w: two tiles) and one past it."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    n, m = A.shape[0], 12
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, 1j * ref.OMEGA_TARGET, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.ResolventBasis(hip_ctx, op, m)
    basis.set_start(ref.start_vector(n))
    Tfull = np.zeros((m + 1, m), order="F")
    assert basis.extend(0, m, Tfull) == -1
    V = basis.basis(m + 1)
    st = op.stats()
    del basis, op
    T = Tfull[:m, :m]
    assert np.array_equal(T, T.T) and np.count_nonzero(np.triu(T, 2)) == 0
    assert (np.diag(Tfull, -1) > 0.0).all()
    orth, defect, tn = basis_checks("S2k", Tfull, V, m)
    print(f"|V^H M V - I|_max = {orth:.2e}; relation defect / |T|_F = {defect / tn:.2e}; refined solves {st['refined_solves']}")
    assert orth <= 1e-12
    assert defect <= 1e-10 * tn


@pytest.mark.parametrize("case,ncv", [("S2k", 12), ("S5k", 20)])
def test_fused_kernels_against_the_unfused_form(tmp_path, case, ncv):
    """The same steps in two child processes, the fused kernels and LSA_LANCZOS_FUSED=0 (k_multi_dot + k_multi_axpy + the tail): T
    and V byte for byte alike.  S5k with ncv = 20 needs three column tiles."""
    fused = run_child("basis", case, ncv, tmp_path / "fused.npz")
    plain = run_child("basis", case, ncv, tmp_path / "plain.npz", LSA_LANCZOS_FUSED="0")
    assert int(fused["bd"]) == -1 and int(plain["bd"]) == -1
    dT, dV = np.abs(plain["T"] - fused["T"]).max(), np.abs(plain["V"] - fused["V"]).max()
    print(f"{case}: fused against unfused: |dT|_max = {dT:.2e}, |dV|_max = {dV:.2e}")
    assert np.array_equal(fused["T"], plain["T"])
    assert np.array_equal(fused["V"], plain["V"])


_SOLVED = {}


def solved(omega):
    """One front-end solve per frequency and process: S2k, num_modes 4, ncv 12, atol 1e-10."""
    if omega not in _SOLVED:
        from Solver.resolvent import ResolventConfig, ResolventSolver

        A, M = ref.case("S2k")
        rs = ResolventSolver(A, M, ResolventConfig(num_modes=4, ncv=12, atol=1e-10))
        _SOLVED[omega] = rs.solve(omega)
        rs.release()
    return _SOLVED[omega]


@pytest.mark.parametrize("omega", ref.OMEGAS)
def test_gains_against_dense(omega):
    """|sigma_j - sigma_j^dense| <= 1e-10 sigma_1 (the symmetric path's bound for Hermitian Ritz values at this tolerance; the numpy
    restatement reaches 1e-15); the iteration restarts (the restatement: 4 to 9 times), so the restart kernels run.  omega = 0 runs on
    real factors with complex vectors."""
    res = solved(omega)
    dense = ref.dense_gains_svd("S2k", omega)[:4]
    err = np.abs(res.gains - dense).max() if len(res.gains) == 4 else np.inf
    print(f"omega = {omega}: gains {res.gains}, |gain - dense|_max / sigma_1 = {err / dense[0]:.2e}, stats {res.stats}")
    assert len(res.gains) == 4 and (np.diff(res.gains) <= 0.0).all()
    assert err <= 1e-10 * dense[0]
    assert res.stats["restarts"] >= 1
    assert res.stats["adjoint_solves"] >= res.stats["applies"] + 4 and res.stats["forward_solves"] >= res.stats["applies"]


@pytest.mark.parametrize("omega", ref.OMEGAS)
def test_pairs(omega):
    """The same solves: ||Q^H M Q - I||_max and ||F^H M F - I||_max <= 1e-10, ||R M f_j - sigma_j q_j||_M <= 1e-8 sigma_j with R
    applied by SuperLU (the suite's residual bound at this tolerance; the restatement's worst is 2.3e-11), and the largest entry of
    each q_j real positive."""
    res = solved(omega)
    A, M = ref.case("S2k")
    oq, of, resid = ref.pair_checks(A, M, omega, res.gains, res.responses, res.forcings)
    print(f"omega = {omega}: |Q^H M Q - I|_max = {oq:.2e}, |F^H M F - I|_max = {of:.2e}, pair residual = {resid:.2e}")
    assert oq <= 1e-10
    assert of <= 1e-10
    assert resid <= 1e-8
    for q in res.responses.T:
        k = int(np.argmax(np.abs(q)))
        assert q[k].real > 0.0 and abs(q[k].imag) <= 1e-14 * abs(q[k])


def test_sweep_on_one_analysis():
    """sweep() over three frequencies on one solver: gains and responses byte for byte those of three fresh solvers, the second and
    third frequency on the first one's analysis."""
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case("S2k")
    cfg = ResolventConfig(num_modes=4, ncv=12, atol=1e-10)
    omegas = [0.4, ref.OMEGA_TARGET, 1.2]
    rs = ResolventSolver(A, M, cfg)
    swept = rs.sweep(omegas)
    rs.release()
    assert [r.omega for r in swept] == omegas
    assert swept[1].stats["analysis_reused"] and swept[2].stats["analysis_reused"]
    for w, got in zip(omegas, swept):
        fresh = solved(w) if w in _SOLVED else None
        if fresh is None:
            one = ResolventSolver(A, M, cfg)
            fresh = one.solve(w)
            one.release()
        assert np.array_equal(got.gains, fresh.gains), w
        assert np.array_equal(got.responses, fresh.responses), w


def test_two_processes_give_the_same_bytes(tmp_path):
    """S5k, num_modes 6, ncv 16 in two fresh processes: gains, responses and forcings byte for byte alike, the gains the dense ones
    to six decimals."""
    a = run_child("solve", "S5k", 16, tmp_path / "a.npz")
    b = run_child("solve", "S5k", 16, tmp_path / "b.npz")
    print(f"S5k gains {a['gains']}, restarts {int(a['restarts'])}")
    for key in ("gains", "responses", "forcings"):
        assert np.array_equal(a[key], b[key]), key
    assert np.allclose(a["gains"], np.array(ref.GAINS_S5K), rtol=0.0, atol=1e-5)


def test_create_refuses_what_it_cannot_run(hip_ctx):
    """lsa_resolvent_create: LSA_ERR_ARG with a message for an operator in adjoint mode, a projected one, one without M, one with an
    ILU."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    n = A.shape[0]
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    sigma = 1j * ref.OMEGA_TARGET

    def refused(op, word):
        with pytest.raises(ValueError) as info:  # (how the binding reports LSA_ERR_ARG; every other status is an LsaError)
            lsa_hip.ResolventBasis(hip_ctx, op, 12)
        assert not isinstance(info.value, lsa_hip.LsaError) and "lsa_resolvent_create" in str(info.value) and word in str(info.value), str(info.value)

    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, sigma, mode=0, pc_type=2, ksp_rtol=1e-12)
    op.set_adjoint(True)
    refused(op, "adjoint")
    op.set_adjoint(False)
    keep = np.ones(n)
    keep[::7] = 0.0
    op.set_projection(keep)
    refused(op, "projected")
    op.set_projection(None)
    lsa_hip.ResolventBasis(hip_ctx, op, 12)  # (and takes it once both are undone)
    del op
    refused(lsa_hip.ShiftInvertOperator(hip_ctx, dA, None, sigma, mode=0, pc_type=2, ksp_rtol=1e-12), "no M")
    # an ILU needs the ordering the front end gives it: in the natural one the pressure row 2 is a zero pivot and lsa_op_create
    # itself fails, before there is an operator to refuse
    from Solver.utils import _combine, _permute, pivot_safe_rcm

    perm = pivot_safe_rcm(_combine(A, M, sigma))
    dAp, dMp = lsa_hip.CsrMatrix.from_scipy(hip_ctx, _permute(A, perm)), lsa_hip.CsrMatrix.from_scipy(hip_ctx, _permute(M, perm))
    refused(lsa_hip.ShiftInvertOperator(hip_ctx, dAp, dMp, sigma, mode=0, pc_type=1, ilu_levels=2, ksp_rtol=1e-10), "exact LU")
