"""GPU tests of the transposed block product ``lsa_spmm_transpose`` (``CsrMatrix.matmat_transpose``) on S2k (n = 1953, a multiple of no
tile) against scipy: a real and a complex operand, both non-symmetric, ``conj`` on and off, a pass remainder, a full pass and a pass
and a remainder of columns, leading dimensions above n."""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
Z = 0.018 + 0.7379601143282424j  # the bench shift: C = A - Z M is complex
PAD = 3                          # leading dimension n + PAD

_CASE = {}


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def _s2k(hip_ctx):
    """Host and device copies of A (real) and C = A - Z M (complex) of S2k, uploaded once for the module."""
    import lsa_hip
    from synthetic import fem

    if not _CASE:
        es = fem.cylinder_case("S2k")
        A = sp.csr_matrix(es.A.real) if np.iscomplexobj(es.A.data) else sp.csr_matrix(es.A)
        C = sp.csr_matrix((es.A.data - Z * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
        for m in (A, C):
            m.sort_indices()
        assert A.dtype == np.float64 and C.dtype == np.complex128 and A.shape[0] == 1953
        assert abs(A - A.T).max() > 0.0 and abs(C - C.T).max() > 0.0  # (a symmetric operand would not tell A^T from A)
        _CASE.update(n=A.shape[0], A=A, C=C, dA=lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), dC=lsa_hip.CsrMatrix.from_scipy(hip_ctx, C))
    return _CASE


def _block(n, cols, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols)))


def _upload_block(hip_ctx, B, ld, fill=np.nan):
    import lsa_hip

    n, cols = B.shape
    flat = np.full((ld, cols), fill, dtype=np.complex128, order="F")
    flat[:n] = B
    return lsa_hip.DeviceVector.from_numpy(hip_ctx, flat.reshape(-1, order="F"))


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("operand", ["A-real", "C-complex"])
@pytest.mark.parametrize("cols", [1, 8, 13])
def test_spmm_transpose_against_scipy(hip_ctx, operand, cols, conj):
    """``Y = A^T X`` / ``A^H X`` with ``ld = n + 3``: componentwise within ``gamma_k (|A|^T |X|)``, ``k`` = longest column + 2 (the
    entries of an output are added in 8 strided sequences and a tree of three levels: at most that many roundings each); the rows
    between the columns untouched (and never read: they hold NaN in X); two calls give the same bytes; with ``conj`` off a complex
    operand is told from its conjugate."""
    import lsa_hip

    s = _s2k(hip_ctx)
    n, ld = s["n"], s["n"] + PAD
    A, dA = (s["A"], s["dA"]) if operand == "A-real" else (s["C"], s["dC"])
    X = _block(n, cols, seed=cols)
    dX = _upload_block(hip_ctx, X, ld)
    outs = []
    for _ in range(2):
        dY = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(ld * cols, 7.0 - 5.0j))
        dA.matmat_transpose(dX, dY, cols, conj=conj, ldx=ld, ldy=ld)
        outs.append(dY.numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    Y = outs[0].reshape((ld, cols), order="F")
    assert np.all(Y[n:] == 7.0 - 5.0j), "rows between the columns were written"
    op = sp.csr_matrix(A.conj().T if conj else A.T)
    ref = op @ X
    k = int(np.diff(op.indptr).max()) + 2
    bound = gamma(k) * (abs(op) @ np.abs(X))
    err = np.abs(Y[:n] - ref)
    print(f"spmm_transpose {operand} cols={cols} conj={conj}: k={k}, max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.isfinite(Y[:n])) and np.all(err <= bound)
    if operand == "C-complex":
        other = sp.csr_matrix(A.T if conj else A.conj().T) @ X
        assert np.max(np.abs(Y[:n] - other)) > 1e3 * np.max(bound)


def test_spmm_transpose_arguments_are_refused(hip_ctx):
    """The block rules of ``lsa_spmm``: ``LSA_ERR_ARG`` with the condition named, before any launch."""
    import lsa_hip

    s = _s2k(hip_ctx)
    n = s["n"]
    x = lsa_hip.DeviceVector(hip_ctx, 2 * n)
    y = lsa_hip.DeviceVector(hip_ctx, 2 * n)
    with pytest.raises(ValueError, match="lsa_spmm_transpose.*does not fit"):
        s["dA"].matmat_transpose(x, y, 3)                      # three columns in vectors of two
    with pytest.raises(ValueError, match="does not fit"):
        s["dA"].matmat_transpose(x, y, 2, ldx=n - 1, ldy=n)    # ld < n
    with pytest.raises(ValueError, match="alias"):
        s["dA"].matmat_transpose(x, x, 2)
    with pytest.raises(ValueError, match="complex128"):
        s["dA"].matmat_transpose(lsa_hip.DeviceVector(hip_ctx, n, np.float64), y, 1)
    with pytest.raises(ValueError, match="0 columns"):
        s["dA"].matmat_transpose(x, y, 0)
