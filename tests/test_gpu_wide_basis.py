"""GPU suite: Krylov bases wider than the fused kernels take, against extended-precision references.

Two things nothing else compares with an independent reference:

  * the per-stage CGS2 that bases of more than 128 vectors run (``multi_dot_partial_kernel``, ``multi_dot_finish_kernel``,
    ``multi_axpy_kernel`` with j > 128; the fused forms stop at 128 columns and are only ever compared with this path), here
    against the Q factor of the same vectors computed in longdouble;
  * the basis product ``basis_gemm_kernel`` behind ``restart`` and ``ritz_vectors``, whose tile of Q outgrows 64 KB of LDS
    beyond 512 complex basis vectors (tiles of 8 columns up to 512, of 4 columns up to 1024, an argument error beyond),
    here against ``extended_reference.matmul_ext`` with the componentwise bound 2 (m + 3) u |V| |Y|.

The operator of the basis is never applied: vectors enter through ``inject`` (one CGS2 step each) and leave through
``ritz_vectors(m, I, normalise=False)``, a product with columns of the identity, exact in any arithmetic."""

import numpy as np
import pytest
import scipy.sparse as sp

import extended_reference as xr

pytestmark = pytest.mark.gpu

N_QR, M_QR = 720, 600  # two chunks of rows in the dot kernels (512 + 208); the longdouble Q factor takes a few seconds
N_GEMM, NCV_MAX = 1100, 1024  # three chunks of rows; the widest basis the product handles
KS = [1, 8, 9, 17]  # column counts around the tiles of 8 and 4
MS = [1, 7, 8, 9, 512, 513, 600, 1024]


def _operator(ctx, n):
    """(A - sigma I)^-1 for a tridiagonal A: anything non-singular will do, it is never applied"""
    import lsa_hip

    A = sp.diags([np.full(n - 1, -1.0), np.linspace(2.0, 3.0, n), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    dA = lsa_hip.CsrMatrix.from_scipy(ctx, A)
    eye = sp.csr_matrix(((A.indices == np.repeat(np.arange(n), np.diff(A.indptr))).astype(np.float64), A.indices, A.indptr), shape=(n, n))  # the identity on A's pattern
    dI = lsa_hip.CsrMatrix.from_scipy(ctx, eye)
    return lsa_hip.ShiftInvertOperator(ctx, dA, dI, 0.5 + 0.25j, pc_type=2), (dA, dI)


def _random_vectors(seed, n, m):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m)))


def _inject_all(kb, W, count):
    for j in range(count):
        kb.inject(j, W[:, j])


def _read_back(kb, m):
    return kb.ritz_vectors(m, np.eye(m, dtype=np.complex128), normalise=False)


def _cgs2_double(W):
    """numpy double restatement of what ``inject`` does, column by column: two classical Gram-Schmidt projections, then the norm"""
    V = np.zeros_like(W)
    for j in range(W.shape[1]):
        w = W[:, j].copy()
        for _ in range(2):
            w = w - V[:, :j] @ (V[:, :j].conj().T @ w)
        V[:, j] = w / np.linalg.norm(w)
    return V


def _distance(V, Qr, Qi):
    """max over the columns of ||V_c - Q_c||_2, the difference taken in longdouble"""
    dr = np.ascontiguousarray(V.real).astype(xr.LD) - Qr
    di = np.ascontiguousarray(V.imag).astype(xr.LD) - Qi
    return float(np.max(np.sqrt(np.sum(dr * dr + di * di, axis=0))))


@pytest.fixture(scope="module")
def qr_case(hip_ctx):
    """600 seeded vectors of length 720 orthonormalised on the device (columns 129.. by the per-stage CGS2), the same in numpy
    double arithmetic, and their Q factor in longdouble (R with a positive diagonal, as CGS2 leaves it)."""
    import lsa_hip

    W = _random_vectors(31, N_QR, M_QR)
    op, keep = _operator(hip_ctx, N_QR)
    kb = lsa_hip.KrylovBasis(hip_ctx, op, M_QR)
    _inject_all(kb, W, M_QR)
    V = {m: _read_back(kb, m) for m in (129, 200, 600)}
    Qr, Qi = xr.qr_positive_ext(W)
    return {"V": V, "Vd": _cgs2_double(W), "Qr": Qr, "Qi": Qi}


@pytest.mark.parametrize("m", [129, 200, 600])
def test_wide_cgs2_against_longdouble_q(qr_case, m):
    """The first m of 600 vectors: the device's orthonormal basis against the longdouble Q factor.

    The tolerance is measured on the reference side, not on the code under test: ``d_ref`` is the distance from the longdouble
    Q of the SAME column-by-column CGS2 carried out by numpy in double arithmetic (sequential sums); the device sums the same
    products in a tree (chunks of 512 rows, four wavefronts, 64 lanes), so it gets 4 x d_ref.  Likewise for the loss of
    orthogonality max |V^H V - I| (Gram matrix in longdouble).

    Measured on an MI355X (n = 720, the figures this test prints):

        m     distance to Q: numpy double   device      max |V^H V - I|: numpy double   device
        129   4.883e-16                     2.614e-16   9.043e-16                       4.451e-16
        200   4.883e-16                     4.579e-16   9.043e-16                       4.451e-16
        600   1.051e-15                     2.248e-15   9.043e-16                       4.451e-16
    """
    V, Vd, Qr, Qi = qr_case["V"][m], qr_case["Vd"][:, :m], qr_case["Qr"][:, :m], qr_case["Qi"][:, :m]
    assert V.shape == (N_QR, m) and np.all(np.isfinite(V))
    assert np.array_equal(V, qr_case["V"][600][:, :m])  # a narrower read-back is the same basis
    d_ref, d_gpu = _distance(Vd, Qr, Qi), _distance(V, Qr, Qi)
    g_ref, g_gpu = xr.gram_defect_ext(Vd), xr.gram_defect_ext(V)
    print(f"wide CGS2 m={m}: distance to the longdouble Q: numpy double {d_ref:.3e}, device {d_gpu:.3e}; "
          f"max |V^H V - I|: numpy double {g_ref:.3e}, device {g_gpu:.3e}")
    assert d_gpu <= 4.0 * d_ref, (d_gpu, d_ref)
    assert g_gpu <= 4.0 * g_ref, (g_gpu, g_ref)


class _GemmCase:
    def __init__(self, ctx):
        import lsa_hip

        self.W = _random_vectors(32, N_GEMM, NCV_MAX + 1)
        self.op, self.keep = _operator(ctx, N_GEMM)
        self.kb = lsa_hip.KrylovBasis(ctx, self.op, NCV_MAX)
        self.rebuild(NCV_MAX + 1)
        self.V = _read_back(self.kb, NCV_MAX)
        rng = np.random.default_rng(33)
        self.Y = {m: np.asfortranarray(rng.standard_normal((m, max(KS))) + 1j * rng.standard_normal((m, max(KS)))) for m in MS}
        self._ref = {}

    def rebuild(self, count):
        """columns 0 .. count-1 of the basis anew from the same vectors (``restart`` consumes the basis)"""
        _inject_all(self.kb, self.W, count)

    def ref(self, m):
        if m not in self._ref:
            self._ref[m] = xr.matmul_ext(self.V[:, :m], self.Y[m])
        return self._ref[m]

    def check(self, got, m, k, what):
        ref = self.ref(m)
        err = xr.ExtResult(ref.re[:, :k], ref.im[:, :k], ref.absrow[:, :k], ref.lengths[:, :k]).error(got)
        bnd = xr.bound(ref.lengths[:, :k], ref.absrow[:, :k])
        bad = np.argwhere(~(err <= bnd))
        assert bad.size == 0, f"{what} m={m} k={k}: {len(bad)} entries outside the bound, first {bad[:3].tolist()}, worst error/bound {np.nanmax(err / bnd):.3g}"


@pytest.fixture(scope="module")
def gemm_case(hip_ctx):
    return _GemmCase(hip_ctx)


def test_wide_basis_read_back_is_orthonormal(gemm_case):
    """1024 vectors of length 1100: what ``ritz_vectors(1024, I)`` returns is the basis CGS2 built -- unit, mutually orthogonal
    columns (the products below take this read-back as their left factor; a product kernel that dropped or mixed up columns
    beyond the 512th would fail here).  CGS2 keeps ||V^H V - I|| at a small multiple of u for these well-conditioned vectors;
    1e-13 = 450 u leaves room for the 1100-term sums."""
    V = gemm_case.V
    assert V.shape == (N_GEMM, NCV_MAX) and np.all(np.isfinite(V))
    assert np.max(np.abs(V.conj().T @ V - np.eye(NCV_MAX))) <= 1e-13
    for m in (1, 8, 512, 513):  # narrower read-backs (tiles of 8 up to 512 columns, of 4 beyond) are the same columns, bit for bit
        assert np.array_equal(_read_back(gemm_case.kb, m), V[:, :m]), m


@pytest.mark.parametrize("m", MS)
def test_ritz_vectors_product(gemm_case, m):
    for k in KS:
        Y = gemm_case.Y[m][:, :k]
        X = gemm_case.kb.ritz_vectors(m, Y, normalise=False)
        assert X.shape == (N_GEMM, k)
        gemm_case.check(X, m, k, "ritz_vectors")
        assert np.array_equal(X, gemm_case.kb.ritz_vectors(m, Y, normalise=False))  # fixed order of additions


@pytest.mark.parametrize("m", MS)
def test_restart_product(gemm_case, m):
    """``restart(m, Q)``: the basis becomes [V[:, :m] Q, V[:, m]]"""
    for k in (q for q in KS if q <= m):
        gemm_case.rebuild(m + 1)
        if m < NCV_MAX:
            before = _read_back(gemm_case.kb, m + 1)
            assert np.array_equal(before, np.column_stack([gemm_case.V[:, :m], before[:, m]]))  # rebuilt bit for bit
        gemm_case.kb.restart(m, gemm_case.Y[m][:, :k])
        after = _read_back(gemm_case.kb, k + 1)
        gemm_case.check(after[:, :k], m, k, "restart")
        if m < NCV_MAX:
            assert np.array_equal(after[:, k], before[:, m])  # the residual vector moves behind the new columns untouched
        else:  # (column 1024 cannot be read back on its own: it is a unit vector orthogonal to the span of the first 1024)
            assert abs(np.linalg.norm(after[:, k]) - 1.0) <= 1e-14
            assert np.max(np.abs(gemm_case.V.conj().T @ after[:, k])) <= 1e-13
    gemm_case.rebuild(NCV_MAX + 1)  # (restart swaps the two halves of the workspace: every column anew for the tests that follow)


def test_basis_wider_than_the_product_handles_is_refused(hip_ctx):
    """1025 basis vectors: ``lsa_krylov_create`` says so instead of letting a launch fail later; the same for GMRES restarts
    (1024 complex, 2048 real basis vectors)"""
    import lsa_hip

    op, keep = _operator(hip_ctx, 64)
    with pytest.raises(ValueError, match=r"ncv=1025.*at most 1024 basis vectors"):
        lsa_hip.KrylovBasis(hip_ctx, op, NCV_MAX + 1)
    dA = lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.diags([np.full(63, -1.0), np.full(64, 4.0), np.full(63, -1.0)], [-1, 0, 1]).tocsr())
    for dtype, limit in ((np.complex128, 1024), (np.float64, 2048)):
        b = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ones(64, dtype=dtype))
        x = lsa_hip.DeviceVector(hip_ctx, 64, dtype)
        with pytest.raises(ValueError, match=rf"restart={limit + 1}.*at most {limit} basis vectors"):
            lsa_hip.gmres(hip_ctx, dA, None, b, x, rtol=1e-10, restart=limit + 1, maxit=5000)
        its, rr = lsa_hip.gmres(hip_ctx, dA, None, b, x, rtol=1e-10, restart=limit, maxit=5000)  # the limit itself is fine
        assert rr <= 1e-10 and its <= 64
