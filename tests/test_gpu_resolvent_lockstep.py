"""GPU suite of the lockstep resolvent sweep: ``lsa_spmv_batch``, ``lsa_resolvent_extend_batch``, ``lsa_resolvent_solve_batch`` and
``ResolventSolver.sweep / norm_map(lockstep=True)`` on the small cylinder case S2k (n = 1953: no multiple of 256, the last chunk of
every reduction is partial).  The claim is identical arithmetic, so every comparison is byte for byte (``tobytes()``): each member of a
group returns what its solo solve returns."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import resolvent_reference as ref
import weighted_reference as wref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
NEV, NCV, TOL = 4, 12, 1e-10
KEYS = ("theta", "gains", "responses", "forcings", "estimates")
_PAIR = {}


def pair():
    if "S2k" not in _PAIR:
        _PAIR["S2k"] = on_shared_pattern(*ref.case("S2k"))
    return _PAIR["S2k"]


def same_bytes(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.tobytes() == b.tobytes())


def open_basis(ctx, dA, dM, shift, ncv=NCV, rtol=1e-12, spoil=False):
    import lsa_hip

    if spoil:
        os.environ["LSA_ND_TEST_PERTURB"] = "1e-7"
    try:
        op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, shift, mode=0, pc_type=2, ksp_rtol=rtol)
    finally:
        os.environ.pop("LSA_ND_TEST_PERTURB", None)
    return lsa_hip.ResolventBasis(ctx, op, ncv), op


def assert_member_equals_solo(r, s):
    for k in KEYS:
        assert same_bytes(r[k], s[k]), k
    assert r["applies"] == s["applies"] and r["restarts"] == s["restarts"] and r["nconv"] == s["nconv"]


# ---- 1. the batched forward product -----------------------------------------------------------------------------------------------
def _spmv_case(ctx, mats, dtype, same_slot=False):
    import lsa_hip

    rng = np.random.default_rng(3)
    n = mats[0].shape[0]
    dm = [lsa_hip.CsrMatrix.from_scipy(ctx, m) for m in mats]
    if same_slot:
        dm = [dm[0]] * len(mats)
    xs = [rng.standard_normal(n) + (1j * rng.standard_normal(n) if dtype == np.complex128 else 0.0) for _ in mats]
    dx = [lsa_hip.DeviceVector.from_numpy(ctx, np.asarray(x, dtype=dtype)) for x in xs]
    solo, batched = [lsa_hip.DeviceVector(ctx, n, dtype) for _ in mats], [lsa_hip.DeviceVector(ctx, n, dtype) for _ in mats]
    for m, x, y in zip(dm, dx, solo):
        m.matvec(x, y)
    lsa_hip.CsrMatrix.spmv_batch(dm, dx, batched)
    for z, (a, b) in enumerate(zip(solo, batched)):
        ya, yb = a.numpy(), b.numpy()
        assert np.isfinite(ya).all() and np.abs(ya).max() > 0.0
        assert ya.tobytes() == yb.tobytes(), f"problem {z} of {len(mats)}"


@pytest.mark.parametrize("J", [1, 3, 16])
@pytest.mark.parametrize("kind", ["f64_c128", "c128_c128", "f64_f64"])
def test_spmv_batch_has_spmvs_bits(hip_ctx, J, kind):
    """J matrices with different values on the S2k pattern (n = 1953, 28 entries a row: sub-waves of 16 lanes), each against
    ``matvec``: real matrix with complex vectors (the weights' products), complex with complex (C_k w_k), real with real."""
    A, M = pair()
    mats = [(M * (1.0 + 0.25 * z)).tocsr() if kind != "c128_c128" else (A - (0.1 + 1j * (0.3 + 0.2 * z)) * M).tocsr() for z in range(J)]
    _spmv_case(hip_ctx, mats, np.float64 if kind == "f64_f64" else np.complex128)


def test_spmv_batch_same_matrix_in_every_slot(hip_ctx):
    """Q x_k for all members of a group: one matrix, five vectors."""
    _, M = pair()
    _spmv_case(hip_ctx, [M] * 5, np.complex128, same_slot=True)


@pytest.mark.parametrize("n,longest", [(37, 37), (97, 80)])
def test_spmv_batch_hand_made_patterns(hip_ctx, n, longest):
    """Hand-made patterns with an empty row and a long row.  A square matrix of 37 columns cannot hold a row of more than 37 entries,
    so n = 37 has a full row (its lanes make several trips) and n = 97 has the row of 80 > 64 entries, longer than a wavefront; the
    short mean row length also picks narrower sub-waves than S2k's."""
    rng = np.random.default_rng(n)
    rows, cols = [], []
    for r in range(n):
        if r == 5:
            continue  # the empty row
        c = np.arange(longest) if r == 11 else np.unique(np.r_[r, rng.integers(0, n, size=int(rng.integers(1, 6)))])
        rows += [r] * len(c)
        cols += list(c)
    P = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    P.sort_indices()
    assert P.indptr[6] == P.indptr[5] and P.indptr[12] - P.indptr[11] == longest
    for dtype in (np.float64, np.complex128):
        mats = []
        for z in range(3):
            Q = P.copy()
            Q.data = rng.standard_normal(P.nnz)
            mats.append(Q)
        _spmv_case(hip_ctx, mats, dtype)
    mats = []
    for z in range(3):
        Q = P.astype(np.complex128)
        Q.data = rng.standard_normal(P.nnz) + 1j * rng.standard_normal(P.nnz)
        mats.append(Q)
    _spmv_case(hip_ctx, mats, np.complex128)


_LARGE = {}


def _large_pattern(form):
    """Patterns of at least 4 Mi entries, where ``k_spmv`` leaves the plain sub-wave rows.  ``group``: n = 150 000 in node blocks
    of three rows with one pattern (4.5 M entries): the row-group kernel for real and complex values.  ``band``: n = 300 000 with 15
    entries a row and no two rows alike (grouping does not pay): the 16-bit column offsets for complex values."""
    if form not in _LARGE:
        if form == "group":
            B = sp.diags([np.ones(50_000 - abs(k)) for k in range(-5, 5)], list(range(-5, 5)), format="csr")
            P = sp.kron(B, np.ones((3, 3)), format="csr")
        else:
            P = sp.diags([np.ones(300_000 - abs(k)) for k in range(-7, 8)], list(range(-7, 8)), format="csr")
        P.sort_indices()
        assert P.nnz >= 4 << 20
        _LARGE[form] = P
    return _LARGE[form]


@pytest.mark.parametrize("form,kind,kernel", [("group", "f64_c128", "spmv_group_kernel"), ("group", "c128_c128", "spmv_group_kernel"),
                                              ("band", "c128_c128", "spmv_subwave16_kernel")])
def test_spmv_batch_on_large_patterns_takes_spmvs_row_form(hip_ctx, form, kind, kernel):
    """The two forms no small pattern reaches, each against ``matvec``, which must itself be running that form (``matvec_info``):
    three slots, two matrices with different values and the first one again."""
    import lsa_hip

    P = _large_pattern(form)
    rng = np.random.default_rng(11)
    n, dtype = P.shape[0], np.complex128
    mats = []
    for z in range(2):
        Q = P.astype(np.complex128 if kind == "c128_c128" else np.float64)
        Q.data = rng.standard_normal(P.nnz) + (1j * rng.standard_normal(P.nnz) if kind == "c128_c128" else 0.0)
        mats.append(lsa_hip.CsrMatrix.from_scipy(hip_ctx, Q))
    dm = [mats[0], mats[1], mats[0]]
    for m in mats:
        assert m.matvec_info(dtype)["kernel"].startswith(kernel), m.matvec_info(dtype)["kernel"]
    dx = [lsa_hip.DeviceVector.from_numpy(hip_ctx, rng.standard_normal(n) + 1j * rng.standard_normal(n)) for _ in dm]
    solo, batched = [lsa_hip.DeviceVector(hip_ctx, n, dtype) for _ in dm], [lsa_hip.DeviceVector(hip_ctx, n, dtype) for _ in dm]
    for m, x, y in zip(dm, dx, solo):
        m.matvec(x, y)
    lsa_hip.CsrMatrix.spmv_batch(dm, dx, batched)
    for z, (a, b) in enumerate(zip(solo, batched)):
        ya, yb = a.numpy(), b.numpy()
        assert np.isfinite(ya).all() and np.abs(ya).max() > 0.0
        assert ya.tobytes() == yb.tobytes(), f"problem {z}"
    assert solo[0].numpy().tobytes() != solo[2].numpy().tobytes()  # (the same matrix, another vector: the slots are not mixed up)


# ---- 2. the batched step kernels, through lsa_resolvent_extend_batch --------------------------------------------------------------
def _extend_case(ctx, A, M, omegas, j0s, m):
    import lsa_hip

    n = A.shape[0]
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    v0 = ref.start_vector(n)
    solo = []
    for w in omegas:
        b, op = open_basis(ctx, dA, dM, 1j * w, ncv=m)
        b.set_start(v0)
        T = np.zeros((m + 1, m), order="F")
        assert b.extend(0, m, T) == -1
        solo.append((T, b.basis(m + 1)))
        del b, op
    objs = [open_basis(ctx, dA, dM, 1j * w, ncv=m) for w in omegas]
    Ts = [np.zeros((m + 1, m), order="F") for _ in omegas]
    for (b, _), j0, T in zip(objs, j0s, Ts):
        b.set_start(v0)
        if j0 > 0:
            assert b.extend(0, j0, T) == -1  # alone to its own column
    bd, status = lsa_hip.ResolventBasis.extend_batch([o[0] for o in objs], j0s, m, Ts)
    assert bd == [-1] * len(omegas) and status == [0] * len(omegas)
    for (b, _), T, (Ts_, Vs) in zip(objs, Ts, solo):
        assert T.tobytes() == Ts_.tobytes()
        assert b.basis(m + 1).tobytes() == Vs.tobytes()
    del objs


def test_extend_batch_members_at_different_columns(hip_ctx):
    """Three S2k bases started at columns 0, 3 and 9: the per-problem ncols of a round are 1, 4, 10 -> ... -> 12, on both sides of
    the column tile of eight; T and the 13 basis columns equal those of twelve solo steps."""
    A, M = pair()
    _extend_case(hip_ctx, A, M, (0.4, 0.8, 1.6), (0, 3, 9), 12)


def test_extend_batch_one_partial_chunk(hip_ctx):
    """The same on a cut-down cylinder mesh with n = 210 < 256: every reduction is one partial chunk."""
    from synthetic import fem

    es = fem.assemble_linearized_ns(fem.channel_mesh(6, 3, grading=fem.GRADING), 50.0)
    A, M = on_shared_pattern(es.A.tocsr(), es.M.tocsr())
    assert 8 < A.shape[0] < 256
    _extend_case(hip_ctx, A, M, (0.4, 0.8, 1.6), (0, 3, 9), 12)


# ---- 3, 4, 7, 8, 10, 11. the front end ---------------------------------------------------------------------------------------------
CFG = dict(num_modes=NEV, ncv=NCV, atol=TOL)
_SEQ = {}


def fresh(**kw):
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case("S2k")
    return ResolventSolver(A, M, ResolventConfig(**CFG), **kw)


def sequential(omegas, **kw):
    """The sequential sweep's results by frequency and solver arguments, computed once and shared."""
    key = tuple(sorted((k, repr(v) if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items()))
    missing = [w for w in omegas if (key, w) not in _SEQ]
    if missing:
        rs = fresh(**kw)
        for w, r in zip(missing, rs.sweep(missing)):
            _SEQ[(key, w)] = r
        rs.release()
    return [_SEQ[(key, w)] for w in omegas]


def assert_results_equal(lock, seq):
    assert len(lock) == len(seq)
    for a, b in zip(lock, seq):
        assert a.omega == b.omega and a.discount == b.discount
        for k in ("gains", "responses", "forcings", "estimates"):
            assert same_bytes(getattr(a, k), getattr(b, k)), (a.omega, k)
        for k in ("applies", "restarts", "nconv", "adjoint_solves", "forward_solves", "refinements"):
            assert a.stats[k] == b.stats[k], (a.omega, k)


OMEGAS5 = (0.3, 0.5, ref.OMEGA_TARGET, 1.0, 1.4)


def test_sweep_lockstep_equals_sequential():
    rs = fresh()
    lock = rs.sweep(OMEGAS5, lockstep=True)
    info = rs.last_lockstep_info
    rs.release()
    print("info:", info, [r.stats for r in lock])
    assert_results_equal(lock, sequential(OMEGAS5))
    assert len(info) == 1
    for r in lock:
        assert r.stats["lockstep"] is True and r.stats["lockstep_steps"] > 0
        assert r.stats["lockstep_steps"] + r.stats["solo_steps"] == r.stats["applies"]
    assert 0 < info[0]["rounds"] < sum(r.stats["applies"] for r in lock)
    assert info[0]["launches_per_round"] > 12


@pytest.mark.parametrize("J", [1, 16, 17])
def test_sweep_of_one_sixteen_and_seventeen(J):
    """One frequency (the solo path), sixteen (every slot of the argument records) and seventeen (chunks of 16 + 1)."""
    omegas = tuple(0.25 + 0.09 * k for k in range(J))
    rs = fresh()
    lock = rs.sweep(omegas, lockstep=True, max_batch=16)
    info = rs.last_lockstep_info
    rs.release()
    assert_results_equal(lock, sequential(omegas))
    assert len(info) == (0 if J == 1 else 1)
    if J >= 16:
        assert all(r.stats["lockstep"] for r in lock[:16]) and info[0]["lockstep_steps"][15] > 0
    if J == 17:
        assert lock[16].stats["lockstep"] is False


def test_sweep_with_a_real_shift_member():
    """omega = 0 under a positive discount is a real shift: real factors, the solo path; the other two run in lockstep."""
    omegas = (0.0, 0.5, 1.0)
    rs = fresh(discount=0.05)
    lock = rs.sweep(omegas, lockstep=True)
    rs.release()
    assert lock[0].stats["lockstep"] is False and lock[1].stats["lockstep"] is True and lock[2].stats["lockstep"] is True
    assert_results_equal(lock, sequential(omegas, discount=0.05))


def test_sweep_with_windows():
    kw = dict(forcing_window=wref.region("S2k", wref.OMEGA_F), response_window=wref.region("S2k", wref.OMEGA_Q))
    omegas = (0.4, ref.OMEGA_TARGET, 1.1)
    rs = fresh(**kw)
    lock = rs.sweep(omegas, lockstep=True)
    rs.release()
    assert all(r.stats["lockstep"] for r in lock)
    assert_results_equal(lock, sequential(omegas, **kw))


def test_memory_budget_cuts_the_group(monkeypatch):
    """Per-member bytes set to 1 / 2.5 of the budget: five frequencies run as 2 + 2 + 1."""
    from Solver.resolvent import ResolventSolver

    monkeypatch.setattr(ResolventSolver, "_lockstep_bytes_per_member", lambda self, prep: int(0.8 * prep["ctx"].mem_info()[0] / 2.5))
    rs = fresh()
    lock = rs.sweep(OMEGAS5, lockstep=True)
    info = rs.last_lockstep_info
    rs.release()
    assert [r.stats.get("batch_size") for r in lock] == [2, 2, 2, 2, None] and len(info) == 2
    assert_results_equal(lock, sequential(OMEGAS5))


def test_norm_map_lockstep():
    pts = np.array([[0.02 + 0.5j, 0.05 + 0.7j, 0.1 + 0.9j], [-0.02 + 0.5j, -0.05 + 0.7j, -0.1 + 0.9j]])
    rs = fresh()
    plain = rs.norm_map(pts, warm_start=False)
    lock = rs.norm_map(pts, warm_start=False, lockstep=True)
    stats = rs.last_map_stats
    with pytest.raises(ValueError, match="warm"):
        rs.norm_map(pts, warm_start=True, lockstep=True)
    rs.release()
    assert lock.shape == pts.shape and lock.tobytes() == plain.tobytes()
    assert all(s["lockstep"] for s in stats)


# ---- 5, 6, 9, 12. lsa_resolvent_solve_batch ---------------------------------------------------------------------------------------
def _solo_and_batch(ctx, omegas, nevs, max_its=500, rtol=1e-12, spoil=(), weights=None):
    """``(solo results, batch results, info, solo operator stats, batch operator stats)`` of the same members."""
    import lsa_hip

    A, M = pair()
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    v0 = ref.start_vector(A.shape[0])
    per = lambda x, z: x[z] if isinstance(x, (tuple, list)) else x  # noqa: E731
    solo, solo_stats = [], []
    for z, w in enumerate(omegas):
        b, op = open_basis(ctx, dA, dM, 1j * w, rtol=rtol, spoil=z in spoil)
        if weights and weights[z] is not None:
            b.set_weights(*weights[z](dM))
        try:
            solo.append(b.solve(per(nevs, z), TOL, per(max_its, z), v0=v0, max_out=NEV))
        except ValueError as exc:
            solo.append(exc)
        solo_stats.append(op.stats())
        del b, op
    objs = [open_basis(ctx, dA, dM, 1j * w, rtol=rtol, spoil=z in spoil) for z, w in enumerate(omegas)]
    for z, (b, _) in enumerate(objs):
        if weights and weights[z] is not None:
            b.set_weights(*weights[z](dM))
    res, info = lsa_hip.ResolventBasis.solve_batch([o[0] for o in objs], nevs, TOL, max_its, v0s=v0, max_out=NEV, raise_on_error=False)
    stats = [o[1].stats() for o in objs]
    del objs
    print("info:", info)
    return solo, res, info, solo_stats, stats


def test_members_at_different_steps_leave_at_different_times(hip_ctx):
    omegas, nevs = (0.4, 0.8, 1.6), (1, 3, 4)
    solo, res, info, _, _ = _solo_and_batch(hip_ctx, omegas, nevs)
    applies = [r["applies"] for r in res]
    print("applies:", applies)
    assert len(set(applies)) > 1  # (a condition on the inputs: the members do not all make the same number of applies)
    for z in range(3):
        assert_member_equals_solo(res[z], solo[z])
        assert info["lockstep_steps"][z] + info["solo_steps"][z] == applies[z] and info["solo_steps"][z] == 0
    assert max(applies) <= info["rounds"] < sum(applies)


def test_one_spoilt_member_refines_alone(hip_ctx):
    """The middle operator's factors are spoilt (LSA_ND_TEST_PERTURB): its first checks miss ksp_rtol, it switches its refinement
    steps on and redoes that step and all later ones alone; the others never leave the rounds."""
    solo, res, info, _, stats = _solo_and_batch(hip_ctx, (0.4, 0.8, 1.6), 3, rtol=1e-8, spoil=(1,))
    assert res[1]["refined_adjoint"] + res[1]["refined_forward"] > 0 and info["solo_steps"][1] > 0
    for z in (0, 2):
        assert info["solo_steps"][z] == 0 and info["lockstep_steps"][z] > 0 and stats[z]["refined_solves"] == 0
    for z in range(3):
        assert_member_equals_solo(res[z], solo[z])
        assert all(res[z][k] == solo[z][k] for k in ("adjoint_solves", "forward_solves", "refined_adjoint", "refined_forward"))


def test_a_member_that_does_not_converge_returns_its_partial_result(hip_ctx):
    solo, res, info, _, _ = _solo_and_batch(hip_ctx, (0.4, 0.8, 1.6), NEV, max_its=(500, 0, 500))
    assert res[1]["nconv"] < NEV and solo[1]["nconv"] == res[1]["nconv"]
    for z in range(3):
        assert_member_equals_solo(res[z], solo[z])
    assert res[0]["nconv"] >= NEV and res[2]["nconv"] >= NEV


def test_a_failing_member_is_named_and_the_others_complete(hip_ctx):
    """The middle handle carries a response weight of zeros (a window that shares M's pattern): no start vector has a positive norm in
    it, which the library reports for that problem alone."""
    import lsa_hip

    zeros = lambda dM: (None, dM.windowed(np.zeros(dM.shape[0])))  # noqa: E731
    solo, res, info, _, _ = _solo_and_batch(hip_ctx, (0.4, 0.8, 1.6), 3, weights=(None, zeros, None))
    assert isinstance(solo[1], ValueError)
    assert isinstance(res[1], (ValueError, lsa_hip.LsaError)) and "problem 1" in str(res[1])
    for z in (0, 2):
        assert_member_equals_solo(res[z], solo[z])


def test_argument_errors_of_a_group(hip_ctx):
    """LSA_ERR_ARG with a text, before any device work: J outside [1, 16], a null handle, a handle given twice, differing ncv, handles
    of another context, F_out without Q_out."""
    import ctypes

    import lsa_hip

    A, M = pair()
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    (b0, op0), (b1, op1), (b2, op2) = (open_basis(hip_ctx, dA, dM, 1j * w, ncv=m) for w, m in ((0.4, NCV), (0.8, NCV), (1.2, NCV + 1)))
    solve = lambda bases, **kw: lsa_hip.ResolventBasis.solve_batch(bases, 2, TOL, 500, max_out=2, **kw)  # noqa: E731
    with pytest.raises(ValueError, match=r"outside \[1, 16\]"):
        solve([b0] * 17)
    with pytest.raises(ValueError, match=r"outside \[1, 16\]"):
        solve([], ctx=hip_ctx)
    with pytest.raises(ValueError, match="share a handle"):
        solve([b0, b1, b0])
    with pytest.raises(ValueError, match="another shape"):
        solve([b0, b2])
    lib, J = hip_ctx._lib, 2
    arr = lambda ptrs: (ctypes.c_void_p * J)(*ptrs)  # noqa: E731
    T = [np.zeros((NCV + 1, NCV), order="F") for _ in range(J)]
    j0, bd, st = (ctypes.c_int32 * J)(0, 0), (ctypes.c_int32 * J)(), (ctypes.c_int32 * J)()
    other = lsa_hip.Context(0)
    try:
        rc = lib.lsa_resolvent_extend_batch(other.handle, 1, arr([b0.handle.value, None]), None, j0, NCV, arr([t.ctypes.data for t in T]), NCV + 1, bd, st)
        assert rc == -1 and "another context" in lib.lsa_last_error(other.handle).decode()
    finally:
        other.close()
    rc = lib.lsa_resolvent_extend_batch(hip_ctx.handle, J, arr([b0.handle.value, None]), None, j0, NCV, arr([t.ctypes.data for t in T]), NCV + 1, bd, st)
    assert rc == -1 and "null handle (problem 1)" in lib.lsa_last_error(hip_ctx.handle).decode()
    # F_out[z] without Q_out[z]
    o = [lsa_hip._ks_options(2, TOL, 500) for _ in range(J)]
    F = [np.zeros((A.shape[0], 2), dtype=np.complex128, order="F") for _ in range(J)]
    th, g = [np.zeros(2) for _ in range(J)], [np.zeros(2) for _ in range(J)]
    res = (lsa_hip.lsa_ks_result * J)()
    rc = lib.lsa_resolvent_solve_batch(hip_ctx.handle, J, arr([b0.handle.value, b1.handle.value]), arr([ctypes.addressof(x) for x in o]), None, 2,
                                       arr([a.ctypes.data for a in th]), arr([a.ctypes.data for a in g]), None, arr([a.ctypes.data for a in F]), None,
                                       ctypes.byref(res), None, ctypes.byref(st), None)
    assert rc == -1 and "F_out needs Q_out" in lib.lsa_last_error(hip_ctx.handle).decode()
    del b0, b1, b2, op0, op1, op2


def test_fused_form_off_runs_every_member_alone():
    """LSA_LANCZOS_FUSED=0 is read once per process: in a child, no member enters the lockstep set and all equal solo."""
    env = dict(os.environ, LSA_LANCZOS_FUSED="0")
    p = subprocess.run([sys.executable, str(HERE / "resolvent_lockstep_child.py")], check=True, env=env, timeout=600, capture_output=True, text=True)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(out)
    assert out["same"] is True
    assert out["info"]["lockstep_steps"] == [0, 0, 0] and out["info"]["rounds"] == 0
    assert out["info"]["solo_steps"] == out["applies"]


def test_fused_form_on_in_the_same_child():
    """The same child with the default: the counter-check that the child does enter the rounds."""
    p = subprocess.run([sys.executable, str(HERE / "resolvent_lockstep_child.py")], check=True, timeout=600, capture_output=True, text=True)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["same"] is True and all(s > 0 for s in out["info"]["lockstep_steps"]) and out["info"]["solo_steps"] == [0, 0, 0]
