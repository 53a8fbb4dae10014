"""GPU suite: forcing / response windows and weights, discounting and the norm map of the resolvent analysis, and the response weight
of transient growth (``lsa_csr_window``, ``lsa_resolvent_set_weights``, ``lsa_growth_set_response_weight``, ``Solver.resolvent``,
``Solver.growth``) on the synthetic cylinder case S2k (n = 1953: no multiple of 256, the last chunk of every reduction is partial), S5k
once for the process-to-process comparison.  References: the dense values and host restatements of ``tests/weighted_reference.py``,
which ``test_weighted_cpu.py`` pins; the bounds are those of ``test_gpu_resolvent.py``, ``test_gpu_growth.py`` and
``test_gpu_growth_sdirk.py`` for the same quantities."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import growth_reference as gref
import growth_sdirk_reference as sref
import resolvent_reference as rref
import weighted_reference as ref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
CASE = "S2k"


def run_child(job, case, ncv, out, **env):
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, str(HERE / "weighted_child.py"), job, case, str(ncv), str(out)], check=True, env=e, timeout=600)
    return np.load(out)


def value_error_naming(info, name):
    """How the binding reports LSA_ERR_ARG: a plain ValueError (every other status is an LsaError) whose text names the function."""
    import lsa_hip

    return not isinstance(info.value, lsa_hip.LsaError) and name in str(info.value)


# ---- 1. lsa_csr_window -----------------------------------------------------------------------------------------------------------------
def test_windowed_values_are_scipys_bits(hip_ctx):
    """A 0/1 window, a tanh window, distinct left and right, and ones: the downloaded values are those of scipy's
    diags(l) @ M @ diags(r) bit for bit (ones: M's own values), the SpMV kernel form is M's, and the product agrees with the host to
    1e-13 of the largest entry."""
    import lsa_hip

    _, M = ref.case(CASE)
    M = sp.csr_matrix(M)
    M.sort_indices()
    n = M.shape[0]
    x, y = ref.dof_xy(CASE)
    box, smooth = ref.window(CASE, *ref.OMEGA_F), 0.5 * (1.0 + np.tanh(x - 2.0))
    dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    rng = np.random.default_rng(0)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    dv, dy = lsa_hip.DeviceVector.from_numpy(hip_ctx, v), lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
    for name, left, right in (("box", box, None), ("tanh", smooth, None), ("left-right", smooth, 1.0 + y * y), ("ones", np.ones(n), None)):
        W = dM.windowed(left, right)
        got = sp.csr_matrix((W.values(), M.indices, M.indptr), shape=M.shape)
        want = sp.diags(left) @ M @ sp.diags(left if right is None else right)
        assert np.array_equal(got.toarray(), want.toarray()), name
        assert W.matvec_info()["kernel"] == dM.matvec_info()["kernel"], name
        W.matvec(dv, dy)
        host = ref.weighted(M, left, right) @ v
        err = np.abs(dy.numpy() - host).max() / np.abs(host).max()
        print(f"{name}: |W v - host|_max / |host|_max = {err:.2e}")
        assert err <= 1e-13, name
        if name == "ones":
            assert np.array_equal(W.values(), dM.values())
        del W


def test_windowed_shares_the_row_groups_of_a_large_matrix(hip_ctx):
    """Above 4 Mi entries k_spmv takes the row-group kernel, whose group table the windowed matrix borrows from M: n = 150 000 in
    node blocks of three rows with one pattern, 4.5 M entries.  The values are the host's bit for bit, the kernel form is M's (a group
    kernel), the product agrees with the host to 1e-13 of the largest entry, and M's own product gives the same bytes before the
    window is made and after it is gone (the borrowed table is M's to free)."""
    import lsa_hip

    rng = np.random.default_rng(3)
    nb = 50_000
    B = sp.diags([np.ones(nb - abs(k)) for k in range(-5, 5)], list(range(-5, 5)), format="csr")
    M = sp.kron(B, np.ones((3, 3)), format="csr")
    M.sort_indices()
    M.data = rng.standard_normal(M.nnz)
    n = M.shape[0]
    assert M.nnz >= 4 << 20
    left, right = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 2.0, n)
    v = rng.standard_normal(n)
    dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    dv, dy = lsa_hip.DeviceVector.from_numpy(hip_ctx, v), lsa_hip.DeviceVector(hip_ctx, n, np.float64)
    dM.matvec(dv, dy)
    before = dy.numpy()
    W = dM.windowed(left, right)
    want = ref.weighted(M, left, right)
    assert np.array_equal(W.values(), want.data)
    kernel = W.matvec_info(np.float64)["kernel"]
    assert kernel == dM.matvec_info(np.float64)["kernel"] and kernel.startswith("spmv_group_kernel"), kernel
    W.matvec(dv, dy)
    host = want @ v
    err = np.abs(dy.numpy() - host).max() / np.abs(host).max()
    print(f"{kernel}: |W v - host|_max / |host|_max = {err:.2e}")
    assert err <= 1e-13
    del W
    dM.matvec(dv, dy)
    assert np.array_equal(dy.numpy(), before)


# ---- the front-end solves, one per setting and process ------------------------------------------------------------------------------------
CFG = dict(num_modes=4, ncv=12, atol=1e-10)
_SOLVED = {}


def solver(fbox=None, qbox=None, **kw):
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case(CASE)
    return ResolventSolver(A, M, ResolventConfig(**CFG), forcing_window=ref.region(CASE, fbox), response_window=ref.region(CASE, qbox), **kw)


def solved(beta, omega, fbox, qbox):
    key = (beta, omega, fbox, qbox)
    if key not in _SOLVED:
        rs = solver(fbox, qbox, discount=beta)
        _SOLVED[key] = rs.solve(omega)
        rs.release()
    return _SOLVED[key]


def plain(omega=ref.OMEGA_TARGET):
    return solved(0.0, omega, None, None)


# ---- 2. identity ----------------------------------------------------------------------------------------------------------------------
def test_windows_of_ones_and_weights_equal_to_m_change_no_bit():
    """Windows of ones (lsa_csr_window's values are M's) and forcing_weight = response_weight = M (the upload route) give the gains,
    responses and forcings of the plain solver, array_equal."""
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case(CASE)
    n = A.shape[0]
    want = plain()
    for kw in (dict(forcing_window=np.ones(n), response_window=np.ones(n)), dict(forcing_weight=M, response_weight=M)):
        rs = ResolventSolver(A, M, ResolventConfig(**CFG), **kw)
        got = rs.solve(ref.OMEGA_TARGET)
        rs.release()
        for key in ("gains", "responses", "forcings"):
            assert np.array_equal(getattr(got, key), getattr(want, key)), (sorted(kw), key)
        assert got.discount == 0.0


def test_a_step_has_the_launches_it_had(hip_ctx):
    """Twelve steps through lsa_resolvent_extend with and without both windows: the same number of sparse products."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case(CASE))
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    Qf, Qq = dM.windowed(ref.window(CASE, *ref.OMEGA_F)), dM.windowed(ref.window(CASE, *ref.OMEGA_Q))
    calls = []
    for weights in (None, (Qf, Qq)):
        op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, 1j * ref.OMEGA_TARGET, mode=0, pc_type=2, ksp_rtol=1e-12)
        basis = lsa_hip.ResolventBasis(hip_ctx, op, 12)
        if weights:
            basis.set_weights(*weights)
        basis.set_start(rref.start_vector(A.shape[0]))
        T = np.zeros((13, 12), order="F")
        assert basis.extend(0, 12, T) == -1
        st = op.stats()
        calls.append((st["spmv_calls"], st["refined_solves"]))
        del basis, op
    print(f"(spmv_calls, refined solves) plain {calls[0]}, weighted {calls[1]}")
    assert calls[0][0] == calls[1][0]


# ---- 3. and 4. gains and pairs, discounting --------------------------------------------------------------------------------------------
ROWS = list(ref.GAINS) + [(ref.BETA, 0.0, ref.OMEGA_F, ref.OMEGA_Q)]  # (the last: real factors, complex vectors)


@pytest.mark.parametrize("key", ROWS, ids=lambda k: f"beta{k[0]}-omega{k[1]:.2f}-{'f' if k[2] else 'M'}-{'q' if k[3] else 'M'}")
def test_gains_and_pairs_against_dense(key):
    """|sigma_j - dense| <= 1e-10 sigma_1; ||Q^H Qq Q - I||_max and ||F^H Qf F - I||_max <= 1e-10; ||R Qf f_j - sigma_j q_j||_Qq <=
    1e-8 sigma_j with R applied by SuperLU; the largest entry of each response real positive; at least one restart."""
    beta, omega, fbox, qbox = key
    res = solved(*key)
    dense = ref.dense_gains(CASE, beta, omega, fbox, qbox)[:4]
    if key in ref.GAINS:
        assert np.allclose(dense, np.array(ref.GAINS[key]), rtol=0.0, atol=1e-6)
    err = np.abs(res.gains - dense).max() if len(res.gains) == 4 else np.inf
    A, M = ref.case(CASE)
    oq, of, resid = ref.pair_checks(A, M, complex(beta, omega), res.gains, res.responses, res.forcings, ref.weight_of(CASE, fbox), ref.weight_of(CASE, qbox))
    print(f"{key}: gains {res.gains}, |gain - dense|_max / sigma_1 = {err / dense[0]:.2e}, |Q^H Qq Q - I|_max = {oq:.2e}, "
          f"|F^H Qf F - I|_max = {of:.2e}, pair residual = {resid:.2e}, stats {res.stats}")
    assert res.discount == beta and res.omega == omega
    assert len(res.gains) == 4 and (np.diff(res.gains) <= 0.0).all()
    assert err <= 1e-10 * dense[0]
    assert oq <= 1e-10
    assert of <= 1e-10
    assert resid <= 1e-8
    assert res.stats["restarts"] >= 1
    for q in res.responses.T:
        k = int(np.argmax(np.abs(q)))
        assert q[k].real > 0.0 and abs(q[k].imag) <= 1e-14 * abs(q[k])


# ---- 5. fused against unfused ----------------------------------------------------------------------------------------------------------
def test_fused_kernels_against_the_unfused_form(tmp_path):
    """Twelve weighted steps in two child processes, the fused kernels and LSA_LANCZOS_FUSED=0: T and V byte for byte alike."""
    fused = run_child("basis", CASE, 12, tmp_path / "fused.npz")
    unfused = run_child("basis", CASE, 12, tmp_path / "unfused.npz", LSA_LANCZOS_FUSED="0")
    assert int(fused["bd"]) == -1 and int(unfused["bd"]) == -1
    assert np.array_equal(fused["T"], unfused["T"])
    assert np.array_equal(fused["V"], unfused["V"])


# ---- 6. block forcings -----------------------------------------------------------------------------------------------------------------
def test_block_forcings_with_windows():
    want = solved(0.0, ref.OMEGA_TARGET, ref.OMEGA_F, ref.OMEGA_Q)
    rs = solver(ref.OMEGA_F, ref.OMEGA_Q, block_forcings=True)
    got = rs.solve(ref.OMEGA_TARGET)
    rs.release()
    for key in ("gains", "responses", "forcings"):
        assert np.array_equal(getattr(got, key), getattr(want, key)), key


# ---- 7. sweep --------------------------------------------------------------------------------------------------------------------------
def test_sweep_with_windows_on_one_analysis():
    """Three frequencies on one solver with both windows: the bytes of fresh solvers, the second and third frequency on the first
    one's analysis (and on the windows built for it)."""
    omegas = [0.4, ref.OMEGA_TARGET, 1.2]
    rs = solver(ref.OMEGA_F, ref.OMEGA_Q)
    swept = rs.sweep(omegas)
    rs.release()
    assert [r.omega for r in swept] == omegas
    assert swept[1].stats["analysis_reused"] and swept[2].stats["analysis_reused"]
    for w, got in zip(omegas, swept):
        fresh = solved(0.0, w, ref.OMEGA_F, ref.OMEGA_Q)
        for key in ("gains", "responses", "forcings"):
            assert np.array_equal(getattr(got, key), getattr(fresh, key)), (w, key)


# ---- 8. norm map -----------------------------------------------------------------------------------------------------------------------
def test_norm_map_against_dense():
    """sigma_1 at {-0.05, 0.1} x {0.4, omega_t} and at the real point 0.2: within 1e-8 relative of the dense value with and without
    warm starts, and at most two preparations (the real point is visited last)."""
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case(CASE)
    pts = np.array([complex(b, w) for b in (-0.05, 0.1) for w in (0.4, ref.OMEGA_TARGET)] + [0.2 + 0.0j])
    pts = np.concatenate([pts[-1:], pts[:-1]])  # (given first, visited last)
    dense = np.array([ref.dense_gains(CASE, z.real, z.imag)[0] for z in pts])
    assert abs(dense[0] - ref.GAINS_REAL_SHIFT[0]) <= 1e-6 and abs(dense[4] - ref.GAINS[(ref.BETA, ref.OMEGA_TARGET, None, None)][0]) <= 1e-6
    rs = ResolventSolver(A, M, ResolventConfig(num_modes=2, ncv=12, atol=1e-10))
    maps = {}
    for warm in (True, False):
        maps[warm] = rs.norm_map(pts, warm_start=warm)
        prepared = sum(st["prepared_anew"] for st in rs.last_map_stats)
        print(f"warm_start = {warm}: sigma_1 {maps[warm]}, |rel err|_max = {np.abs(maps[warm] / dense - 1.0).max():.2e}, restarts "
              f"{[st['restarts'] for st in rs.last_map_stats]}, preparations {prepared}")
        assert maps[warm].shape == pts.shape and len(rs.last_map_stats) == pts.size
        assert (np.abs(maps[warm] / dense - 1.0) <= 1e-8).all()
        assert 1 <= prepared <= 2
        assert rs.last_map_stats[0]["prepared_anew"] and not any(st["prepared_anew"] for st in rs.last_map_stats[2:])  # (the real point, then the first complex one)
    rs.release()
    assert (np.abs(maps[True] / maps[False] - 1.0) <= 1e-8).all()


# ---- 9. transient growth ---------------------------------------------------------------------------------------------------------------
GCFG = dict(dt=gref.DT, num_modes=3, ncv=12, atol=1e-10)
_GROWN = {}


def grown(nsteps, qbox=ref.OMEGA_Q, **cfg):
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    key = (nsteps, qbox, tuple(sorted(cfg.items())))
    if key not in _GROWN:
        A, M = ref.case(CASE)
        c = TransientGrowthConfig(**{**GCFG, **cfg})
        tg = TransientGrowthSolver(A, M, c, response_window=ref.region(CASE, qbox))
        _GROWN[key] = tg.solve(nsteps * c.dt)
        tg.release()
    return _GROWN[key]


@pytest.mark.parametrize("nsteps", [16, 40])
def test_growth_gains_against_dense(nsteps):
    """|G_i - G_i^dense| <= 1e-10 G_1 (the bound of test_gpu_growth.py), response_energy = gains to 1e-10 relative and = r^T Q r on the
    host to 1e-12 relative (a sum of n = 1953 terms in double precision), energy still the M-energy curve."""
    res = grown(nsteps)
    dense = ref.dense_growth_gains(CASE, nsteps, ref.OMEGA_Q)[:3]
    assert np.allclose(dense, np.array(ref.GROWTH_GAINS[nsteps]), rtol=0.0, atol=1e-6)
    err = np.abs(res.gains - dense).max() if len(res.gains) == 3 else np.inf
    A, M = ref.case(CASE)
    Q = ref.weight_of(CASE, ref.OMEGA_Q)
    R = res.responses
    host_q, host_m = np.einsum("ic,ic->c", R, Q @ R), np.einsum("ic,ic->c", R, M @ R)
    print(f"N = {nsteps}: gains {res.gains}, |G - dense|_max / G_1 = {err / dense[0]:.2e}, response_energy {res.response_energy}, "
          f"|E_Q / G - 1|_max = {np.abs(res.response_energy / res.gains - 1.0).max():.2e}, |E_Q / r^T Q r - 1|_max = "
          f"{np.abs(res.response_energy / host_q - 1.0).max():.2e}, stats {res.stats}")
    assert len(res.gains) == 3 and (np.diff(res.gains) <= 0.0).all()
    assert err <= 1e-10 * dense[0]
    assert res.stats["restarts"] >= 1
    assert res.response_energy.shape == (3,)
    assert (np.abs(res.response_energy / res.gains - 1.0) <= 1e-10).all()
    assert (np.abs(res.response_energy / host_q - 1.0) <= 1e-12).all()
    assert (np.abs(res.energy[:, nsteps] / host_m - 1.0) <= 1e-12).all() and np.abs(res.energy[:, 0] - 1.0).max() <= 1e-12


def test_growth_window_of_ones_changes_no_bit():
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case(CASE)
    out = []
    for kw in ({}, dict(response_window=np.ones(A.shape[0]))):
        tg = TransientGrowthSolver(A, M, TransientGrowthConfig(**GCFG), **kw)
        out.append(tg.solve(16 * gref.DT))
        tg.release()
    for key in ("gains", "initial", "responses", "energy"):
        assert np.array_equal(getattr(out[0], key), getattr(out[1], key)), key
    assert np.allclose(out[0].gains, np.array(gref.GAINS[(CASE, 16)]), rtol=0.0, atol=1e-6)
    assert (np.abs(out[0].response_energy / out[0].gains - 1.0) <= 1e-10).all()


def test_growth_sdirk2_with_the_window():
    """scheme="sdirk2", dt = 0.5, N = 8 with the response window against the host iteration on the SuperLU two-stage march with Q at
    the turn: |G_i - G_i^host| <= 1e-10 G_1 (the bound of test_gpu_growth_sdirk.py)."""
    N = 8
    res = grown(N, dt=sref.DT, scheme="sdirk2")
    A, M = ref.case(CASE)
    host = ref.TurnedMarch(sref.SdirkMarch(A, M, sref.DT, gref.keep_mask(CASE)), ref.weight_of(CASE, ref.OMEGA_Q))
    want = sref.march_trl(host, N, 3, 12, 1e-10, gref.start_vector(A.shape[0]))["gains"]
    err = np.abs(res.gains - want).max() if len(res.gains) == 3 else np.inf
    print(f"SDIRK2 N = {N}: gains {res.gains}, host {want}, |G - host|_max / G_1 = {err / want[0]:.2e}")
    assert res.scheme == "sdirk2" and len(res.gains) == 3
    assert err <= 1e-10 * want[0]
    assert (np.abs(res.response_energy / res.gains - 1.0) <= 1e-10).all()


def test_growth_fused_march_against_the_unfused_form(tmp_path):
    fused = run_child("growth", CASE, 12, tmp_path / "fused.npz")
    unfused = run_child("growth", CASE, 12, tmp_path / "unfused.npz", LSA_GROWTH_FUSED="0")
    for key in ("gains", "initial", "responses", "energy", "response_energy", "estimates"):
        assert np.array_equal(fused[key], unfused[key]), key
    assert np.array_equal(fused["gains"], grown(16).gains)


# ---- 10. refusals through the C-ABI ----------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_it_cannot_run(hip_ctx):
    import lsa_hip

    A, M = on_shared_pattern(*ref.case(CASE))
    n = A.shape[0]
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    dMc = lsa_hip.CsrMatrix.from_scipy(hip_ctx, M.astype(np.complex128))
    small = lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.identity(7, format="csr"))
    op = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, 1j * ref.OMEGA_TARGET, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.ResolventBasis(hip_ctx, op, 12)
    for kw, word in ((dict(forcing=dMc), "complex"), (dict(response=dMc), "complex"), (dict(forcing=small), "size"), (dict(response=small), "size")):
        with pytest.raises(ValueError) as info:
            basis.set_weights(**kw)
        assert value_error_naming(info, "lsa_resolvent_set_weights") and word in str(info.value), str(info.value)
    basis.set_weights(dM, None)  # (and takes a real matrix of the right size)
    del basis, op
    with pytest.raises(ValueError) as info:
        dMc.windowed(np.ones(n))
    assert value_error_naming(info, "lsa_csr_window") and "complex" in str(info.value)
    bad = np.ones(n)
    bad[n // 2] = np.nan
    for args in ((bad, None), (np.ones(n), bad)):
        with pytest.raises(ValueError) as info:
            dM.windowed(*args)
        assert value_error_naming(info, "lsa_csr_window") and "finite" in str(info.value)
    gop = lsa_hip.ShiftInvertOperator(hip_ctx, dA, dM, 1.0 / gref.DT, mode=0, pc_type=2, ksp_rtol=1e-12)
    gb = lsa_hip.GrowthBasis(hip_ctx, gop, 12, 4, gref.keep_mask(CASE))
    for Q, word in ((dMc, "complex"), (small, "size")):
        with pytest.raises(ValueError) as info:
            gb.set_response_weight(Q)
        assert value_error_naming(info, "lsa_growth_set_response_weight") and word in str(info.value)
    del gb, gop


# ---- 11. two fresh processes -----------------------------------------------------------------------------------------------------------
def test_two_processes_give_the_same_bytes(tmp_path):
    """S5k with both windows, num_modes 4, ncv 16, in two fresh processes: gains, responses and forcings byte for byte alike."""
    a = run_child("solve", "S5k", 16, tmp_path / "a.npz")
    b = run_child("solve", "S5k", 16, tmp_path / "b.npz")
    print(f"S5k windowed gains {a['gains']}, restarts {int(a['restarts'])}")
    assert len(a["gains"]) == 4
    for key in ("gains", "responses", "forcings"):
        assert np.array_equal(a[key], b[key]), key
