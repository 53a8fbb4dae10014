"""CPU suite: the extended-precision references of the kernel tests (``extended_reference``) against exact rational arithmetic
and against themselves -- a reference that was wrong would make every GPU comparison meaningless."""

import numpy as np
import pytest
import scipy.sparse as sp

import extended_reference as xr


def _sparse(seed, cplx):
    rng = np.random.default_rng(seed)
    A = sp.random(40, 40, density=0.15, random_state=seed, format="csr", data_rvs=rng.standard_normal)
    A.data[::5] = 0.0
    if cplx:
        A = A.astype(np.complex128)
        A.data = A.data + 1j * rng.standard_normal(A.nnz)
    A = sp.csr_matrix(A)
    lil = A.tolil()
    lil[3, :] = 0  # an empty row and an empty column
    lil[:, 9] = 0
    A = sp.csr_matrix(lil)
    x = rng.standard_normal(40) + (1j * rng.standard_normal(40) if cplx else 0.0)
    return A, x


def test_longdouble_is_wide_here_or_the_fraction_forms_run():
    assert xr.WIDE == (np.finfo(np.longdouble).nmant >= 63)


@pytest.mark.parametrize("mat_c,vec_c", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("trans", [None, "T", "H"])
def test_spmv_ext_against_exact_rationals(mat_c, vec_c, trans):
    A, _ = _sparse(1, mat_c)
    _, x = _sparse(2, vec_c)
    fast, exact = xr.spmv_ext(A, x, trans), xr.spmv_ext(A, x, trans, force_fraction=True)
    assert fast.is_complex == (mat_c or vec_c) == exact.is_complex
    op = A if trans is None else (A.T if trans == "T" else A.conj().T)
    dense = sp.csr_matrix(op) @ x
    # the longdouble sums agree with the exact ones to 2^-11 of the double bound; numpy's double product is inside the bound
    assert np.all(exact.error(fast.value()) <= exact.bound() / 1024 + 2.0**-53 * np.abs(exact.value()))
    assert np.all(exact.error(dense) <= exact.bound())
    assert np.array_equal(fast.lengths, np.diff(sp.csr_matrix(op).indptr)) and np.array_equal(fast.absrow, exact.absrow)
    empty = fast.lengths == 0
    assert empty.any() and np.all(fast.value()[empty] == 0) and np.all(fast.bound()[empty] == 0)
    # one term dropped from one row is outside the bound
    r = int(np.argmax(fast.lengths))
    wrong = dense.copy()
    wrong[r] += 1e-11 * float(fast.absrow[r])
    assert not np.all(fast.error(wrong) <= fast.bound())
    assert not np.all(fast.error(np.where(np.arange(40) == r, np.nan, dense)) <= fast.bound())  # a row never written


def test_matmul_ext_against_exact_rationals():
    rng = np.random.default_rng(5)
    V = rng.standard_normal((6, 11)) + 1j * rng.standard_normal((6, 11))
    Y = rng.standard_normal((11, 3)) + 1j * rng.standard_normal((11, 3))
    fast, exact = xr.matmul_ext(V, Y), xr.matmul_ext(V, Y, force_fraction=True)
    assert np.all(exact.error(fast.value()) <= exact.bound() / 1024 + 2.0**-53 * np.abs(exact.value()))
    assert np.all(exact.error(V @ Y) <= exact.bound()) and np.all(fast.lengths == 11)
    real = xr.matmul_ext(V.real, Y.real)
    assert not real.is_complex and np.all(real.error(V.real @ Y.real) <= real.bound())


def test_qr_positive_ext_is_the_q_factor():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((90, 60)) + 1j * rng.standard_normal((90, 60))
    Qr, Qi = xr.qr_positive_ext(X, panel=16)
    Q = Qr.astype(np.float64) + 1j * Qi.astype(np.float64)
    assert xr.gram_defect_ext(Q) <= 4 * 2.0**-53  # (orthonormal to longdouble accuracy; what is left is the rounding to double)
    R = Q.conj().T @ X
    assert np.max(np.abs(np.tril(R, -1))) <= 1e-13 and np.all(np.diag(R).real > 0) and np.max(np.abs(np.diag(R).imag)) <= 1e-13
    assert np.linalg.norm(Q @ R - X) <= 1e-13 * np.linalg.norm(X)
