"""GPU suite: the trace of the stochastic-forcing operator by block probes (``csrc/stochastic_trace.hip``, ``lsa_stochastic_trace``,
``lsa_stochastic_probes``, ``lsa_shifted_spmm_transpose``, ``Solver.stochastic``'s ``trace=`` and ``total_variance``) on the synthetic
cylinder case S2k (n = 1953: every chunk and tile of the kernels has a partial tail), band [0, 1.5], ``ksp_rtol = 1e-12``, against the
numpy generator, a long-double product and SuperLU on the host."""

import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import stochastic_reference as ref
import trace_reference as tref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "stochastic_s2k.json").read_text())
U = 2.0**-53
LD = np.longdouble
DENSE_TRACE = 25411.73396  # tr S of S2k, band [0, 1.5], 8 Gauss nodes (dense, on the host; the golden file's eofs_trace)


def random_pair(seed=3):
    """``test_gpu_stochastic.py::random_pair`` restated: two real matrices on one pattern, 96 x 96, 50 rows with entries, one of them
    with 80 (more than 64), the rest between 1 and 9; the columns -- the rows of the transposed product -- are as uneven."""
    rng = np.random.default_rng(seed)
    n = 96
    rows = rng.choice(n, size=50, replace=False)
    indptr, indices = [0], []
    for i in range(n):
        if i in rows:
            count = 80 if i == rows[0] else int(rng.integers(1, 10))
            indices.extend(np.sort(rng.choice(n, size=count, replace=False)).tolist())
        indptr.append(len(indices))
    nnz = len(indices)
    mk = lambda: sp.csr_matrix((rng.standard_normal(nnz), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n))  # noqa: E731
    return mk(), mk()


def long_double_adjoint_product(A, M, z, X):
    """``(y_ref, bound, lengths)``: ``Y[:, c] = (A - z_c M)^H X[:, c]`` summed in long double entry by entry, ``(|A| + |z_c| |M|)^T |X[:, c]|``
    and the number of terms of every output row."""
    n, N = X.shape
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = np.asarray(A.indices, dtype=np.int64)
    a, m = A.data.astype(LD), M.data.astype(LD)
    Y = np.zeros((n, N), dtype=np.clongdouble)
    B = np.zeros((n, N), dtype=LD)
    for c in range(N):
        zr, zi = LD(z[c].real), LD(z[c].imag)
        x = X[rows, c]
        xr, xi = x.real.astype(LD), x.imag.astype(LD)
        cr, ci = a - zr * m, zi * m  # conj(a - z m)
        yr, yi, b = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
        np.add.at(yr, cols, cr * xr - ci * xi)
        np.add.at(yi, cols, cr * xi + ci * xr)
        np.add.at(b, cols, (np.abs(a) + np.sqrt(zr * zr + zi * zi) * np.abs(m)) * np.sqrt(xr * xr + xi * xi))
        Y[:, c] = yr + 1j * yi
        B[:, c] = b
    return Y, B, np.bincount(cols, minlength=n).astype(LD)[:, None]


def s2k_device(hip_ctx):
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    return A, M, lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)


def make_basis(hip_ctx, dA, dM, N, kind="eofs"):
    import lsa_hip

    om, w = ref.gauss_band(*ref.BAND, N)
    basis = lsa_hip.StochasticBasis(hip_ctx, dA, dM, 1j * om, w, 4, ksp_rtol=1e-12)
    basis.set_kind(0 if kind == "eofs" else 1)
    return basis


# ---- 5. the generator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobes", [1, 5])
def test_probes_equal_the_numpy_generator(hip_ctx, nprobes):
    """``lsa_stochastic_probes`` bit for bit the numpy restatement, in the caller's numbering with and without a row permutation."""
    A, M, dA, dM = s2k_device(hip_ctx)
    n = A.shape[0]
    basis = make_basis(hip_ctx, dA, dM, 1)
    want = tref.probes(n, nprobes, seed=7)
    assert np.array_equal(basis.probes(nprobes, seed=7), want)
    basis.set_row_permutation(np.random.default_rng(0).permutation(n).astype(np.int32))
    assert np.array_equal(basis.probes(nprobes, seed=7), want)
    basis.set_row_permutation(None)
    assert np.array_equal(basis.probes(nprobes, seed=2**40 + 1), tref.probes(n, nprobes, seed=2**40 + 1))
    del basis


# ---- 6. the transposed family product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 16, 17, 33])
@pytest.mark.parametrize("which", ["S2k", "random"])
def test_shifted_spmm_transpose_against_long_double(hip_ctx, which, N):
    """``lsa_shifted_spmm_transpose`` componentwise against a long-double product with the bound of
    ``test_gpu_stochastic.py::test_shifted_spmm_against_long_double``: ``|y - y_ref| <= (len + 2) u (|A| + |z_c| |M|)^T |x|``, ``len``
    the entries of the output row (a column of the pattern); an empty one gives an exact zero.  Column ``c`` against
    ``lsa_spmv_transpose`` on ``C_c = A - z_c M`` within the same bound (another summation order: no bit equality)."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k")) if which == "S2k" else random_pair()
    n = A.shape[0]
    rng = np.random.default_rng(N)
    z = rng.standard_normal(N) + 1j * rng.uniform(0.0, 1.5, N)
    X = rng.standard_normal((n, N)) + 1j * rng.standard_normal((n, N))
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    Y = lsa_hip.shifted_spmm_transpose(hip_ctx, dA, dM, z, X)
    Yref, B, lens = long_double_adjoint_product(A, M, z, X)
    err = np.abs(Y.astype(np.clongdouble) - Yref)
    bound = (lens + 2) * LD(U) * B
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{which}, N = {N}: worst |y - y_ref| / bound = {worst:.3f}, output rows of up to {int(lens.max())} entries")
    assert (err <= bound).all()
    assert (Y[lens[:, 0] == 0] == 0.0).all()
    dy = lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
    for c in sorted({0, N // 2, N - 1}):
        C = dA.axpby(dM, 1.0, -z[c], dtype=np.complex128)
        C.rmatvec(lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(X[:, c])), dy, conj=True)
        assert (np.abs(Y[:, c] - dy.numpy()).astype(LD) <= bound[:, c]).all(), c
    with pytest.raises(ValueError, match="lsa_shifted_spmm_transpose"):
        lsa_hip.shifted_spmm_transpose(hip_ctx, dA, lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.csr_matrix(sp.eye(n))), z, X)


# ---- 7. the forms against the host --------------------------------------------------------------------------------------------------
_HOSTS, _MODES = {}, {}


def hosts(N):
    """Two host references of one quadrature: SuperLU with the COLAMD and with the natural column ordering."""
    if N not in _HOSTS:
        A, M = ref.case("S2k")
        om, w = ref.gauss_band(*ref.BAND, N)
        _HOSTS[N] = (ref.HostStochastic(A, M, om, w), ref.HostStochastic(A, M, om, w, permc_spec="NATURAL"))
    return _HOSTS[N]


def front_end_modes(N, kind):
    """4 modes of a front-end solve at ``atol = 1e-10`` (one per configuration and process)."""
    if (N, kind) not in _MODES:
        from Solver.stochastic import StochasticConfig, StochasticForcingSolver

        sf = StochasticForcingSolver(*ref.case("S2k"), StochasticConfig(num_modes=4, ncv=24, atol=1e-10, nodes=N))
        res = sf.solve(band=ref.BAND, kind=kind)
        sf.release()
        assert res.modes.shape[1] == 4
        _MODES[(N, kind)] = res.modes
    return _MODES[(N, kind)]


def host_terms_and_tolerance(N, Z, kind, modes):
    """``(terms, tol)``: the node terms ``z^T Re(W_k p) w_k / pi`` of the COLAMD reference (``N x R``) and, per probe, ten times the
    larger of the spread between the two host references (forms and node terms) and ``1e-12 sum_k |term_k|`` -- ten for the device's
    different elimination order."""
    a, b = hosts(N)
    Ta, Tb = tref.one_column_terms(a, Z, kind, modes), tref.one_column_terms(b, Z, kind, modes)
    scale = np.abs(Ta).sum(axis=0)
    spread = np.maximum(np.abs(Ta - Tb).max(axis=0), np.abs(Ta.sum(axis=0) - Tb.sum(axis=0)))
    print(f"N = {N}, {kind}, deflated {modes is not None}: host spread / sum|term| per probe = {np.array2string(spread / scale, precision=2)}")
    return Ta, 10.0 * np.maximum(spread, 1e-12 * scale)


@pytest.mark.parametrize("deflate", [False, True])
@pytest.mark.parametrize("kind", ["eofs", "optimals"])
@pytest.mark.parametrize("N", [3, 17])
def test_forms_against_the_host_reference(hip_ctx, N, kind, deflate):
    """``basis.trace`` with 5 Gaussian probes of the caller's: ``forms`` and ``node_terms`` against ``z @ HostStochastic.node_vectors(p)
    * c``, within ten times the larger of the spread between two SuperLU references (COLAMD, NATURAL) and ``1e-12 sum_k |term_k|``.
    17 nodes are two runs of factor sets (16 + 1).  The spread measured, with and without deflation: between 1.5e-16 and 2.8e-15 of ``sum_k |term_k|``
    (printed by every run), so the floor governs: the device is held to ``1e-11 sum_k |term_k|`` (and came within 5e-15)."""
    A, M, dA, dM = s2k_device(hip_ctx)
    n = A.shape[0]
    Z = np.random.default_rng(11).standard_normal((n, 5))
    modes = front_end_modes(N, kind) if deflate else None
    want, tol = host_terms_and_tolerance(N, Z, kind, modes)
    basis = make_basis(hip_ctx, dA, dM, N, kind)
    out = basis.trace(5, probes=Z, modes=modes)
    del basis
    err_t = np.abs(out["node_terms"] - want).max(axis=0)
    err_f = np.abs(out["forms"] - want.sum(axis=0))
    print(f"device: |term - ref|_max / tol = {np.array2string(err_t / tol, precision=3)}, |form - ref| / tol = {np.array2string(err_f / tol, precision=3)}; "
          f"stats {out['stats']}")
    assert out["node_terms"].shape == (N, 5)
    assert (err_t <= tol).all() and (err_f <= tol).all()
    sums = np.zeros(5)
    for k in range(N):
        sums += out["node_terms"][k]
    assert np.array_equal(sums, out["forms"])  # (the forms are their columns added in node order)
    st = out["stats"]
    assert st["solves_adjoint" if kind == "eofs" else "solves_forward"] == 2 * N * 5
    assert st["solves_forward" if kind == "eofs" else "solves_adjoint"] == 0


# ---- 8. the same bits -------------------------------------------------------------------------------------------------------------
def test_batch_width_runs_and_given_probes_give_the_same_bits(hip_ctx):
    A, M, dA, dM = s2k_device(hip_ctx)
    basis = make_basis(hip_ctx, dA, dM, 4)
    runs = {b: basis.trace(5, seed=3, batch=b) for b in (2, 8, 0)}
    again = basis.trace(5, seed=3, batch=2)
    given = basis.trace(5, probes=basis.probes(5, seed=3))
    del basis
    for name in ("forms", "node_terms"):
        for other in (runs[8], runs[0], again, given):
            assert np.array_equal(runs[2][name], other[name]), name
    assert runs[2]["stats"]["batch"] == 2 and runs[2]["stats"]["batches"] == 3
    assert runs[8]["stats"]["batch"] == 5 and runs[8]["stats"]["batches"] == 1  # (no more than the probes there are)
    for r in runs.values():
        assert r["stats"]["widest_pass"] == 4 and r["stats"]["grouped_sweeps"] >= 1
        assert r["stats"]["solves_adjoint"] == 2 * 4 * 5
    assert np.abs(runs[2]["forms"]).min() > 0.0


# ---- 9. the refinement branch -----------------------------------------------------------------------------------------------------
def test_forced_refinement_agrees_and_is_counted(hip_ctx):
    A, M, dA, dM = s2k_device(hip_ctx)
    n = A.shape[0]
    N, R = 3, 5
    Z = np.random.default_rng(11).standard_normal((n, R))
    want, tol = host_terms_and_tolerance(N, Z, "eofs", None)
    basis = make_basis(hip_ctx, dA, dM, N)
    plain = basis.trace(R, probes=Z)
    basis.set_refinement(True)
    forced = basis.trace(R, probes=Z)
    del basis
    print(f"forced refinement: |form - plain| / tol = {np.array2string(np.abs(forced['forms'] - plain['forms']) / tol, precision=3)}; stats {forced['stats']}")
    assert (np.abs(forced["forms"] - plain["forms"]) <= tol).all()
    assert (np.abs(forced["node_terms"] - want).max(axis=0) <= tol).all()
    assert forced["stats"]["refined_solves"] == 2 * N * R == forced["stats"]["solves_adjoint"]


# ---- 10. the front end ------------------------------------------------------------------------------------------------------------
def test_front_end_total_variance_and_captured_fractions():
    """``solve(trace=TraceConfig(probes=16, seed=0))`` with 8 nodes and 4 modes: the eigen results bit for bit those without ``trace=``;
    the probes' part of the total against the host reference's deflated forms for the same generated probes within the tolerance of
    ``test_forms_against_the_host_reference``; ``total_variance`` with the same probes and no deflation within 4 of its own standard
    errors of the dense trace (the device generator's seed 0)."""
    from Solver.stochastic import StochasticConfig, StochasticForcingSolver, TraceConfig

    A, M = ref.case("S2k")
    n = A.shape[0]
    cfg = StochasticConfig(num_modes=4, ncv=24, atol=1e-10, nodes=8)
    sf = StochasticForcingSolver(A, M, cfg)
    plain = sf.solve(band=ref.BAND)
    traced = sf.solve(band=ref.BAND, trace=TraceConfig(probes=16, seed=0))
    total, stderr, node_totals = sf.total_variance(band=ref.BAND, probes=16, seed=0)
    sf.release()
    for name in ("variances", "modes", "spectrum", "estimates"):
        assert np.array_equal(getattr(plain, name), getattr(traced, name)), name
    assert plain.total_variance is None and plain.captured is None and "trace" not in plain.stats
    Z = tref.probes(n, 16, seed=0)
    want, tol = host_terms_and_tolerance(8, Z, "eofs", traced.modes)
    rest = traced.total_variance - traced.variances.sum()
    print(f"total {traced.total_variance:.4f} +- {traced.total_variance_stderr:.4f} (dense {DENSE_TRACE}), captured {traced.captured}, "
          f"|rest - host| = {abs(rest - want.sum(axis=0).mean()):.3e} (tolerance {tol.mean():.3e}); undeflated {total:.4f} +- {stderr:.4f}; "
          f"trace stats {traced.stats['trace']}")
    assert abs(rest - want.sum(axis=0).mean()) <= tol.mean()
    assert abs(traced.node_totals.sum() - traced.total_variance) <= 1e-12 * traced.total_variance
    assert traced.node_totals.shape == (8,) and (traced.node_totals > 0.0).all()
    assert (np.diff(traced.captured) > 0.0).all() and 0.0 < traced.captured[-1] < 1.0
    assert traced.captured_stderr.shape == (4,) and traced.total_variance_stderr > 0.0
    assert traced.stats["trace"]["solves_adjoint"] == 2 * 8 * 16
    assert abs(total - DENSE_TRACE) <= 4 * stderr
    assert abs(node_totals.sum() - total) <= 1e-12 * total
    assert abs(GOLDEN["eofs_trace"] - DENSE_TRACE) <= 1e-5


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(hip_ctx):
    import lsa_hip

    A, M, dA, dM = s2k_device(hip_ctx)
    n = A.shape[0]
    basis = make_basis(hip_ctx, dA, dM, 2)

    def refused(word, call):
        with pytest.raises(ValueError) as info:  # (how the binding reports LSA_ERR_ARG; every other status is an LsaError)
            call()
        assert not isinstance(info.value, lsa_hip.LsaError) and "lsa_stochastic_trace" in str(info.value) and word in str(info.value), str(info.value)

    refused("nprobes = 0", lambda: basis.trace(0))
    skewed = np.random.default_rng(2).standard_normal((n, 3))
    refused("not orthonormal", lambda: basis.trace(2, modes=skewed))
    forms, st = np.zeros(2), lsa_hip.lsa_stochastic_trace_stats()
    refused("U is NULL", lambda: basis._call("trace", 2, ctypes.c_uint64(0), None, 3, None, 0, forms.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(st)))
    refused("batch = -1", lambda: basis.trace(2, batch=-1))
    refused("ndeflate = -2", lambda: basis._call("trace", 2, ctypes.c_uint64(0), None, -2, None, 0, forms.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(st)))
    out = basis.trace(2, seed=1)
    del basis
    assert np.isfinite(out["forms"]).all() and (out["forms"] != 0.0).all() and out["stats"]["solves_adjoint"] == 2 * 2 * 2
