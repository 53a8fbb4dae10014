"""Extended-precision references for the kernel tests: sparse and dense products, and the Q factor of a tall matrix.

Independent of ``oracle/`` and of the library: numpy only.  Everything is carried in ``np.longdouble`` (64-bit significand
on x86), complex numbers as separate real and imaginary longdouble arrays (numpy's ``clongdouble`` product is free to fuse
and reorder; the four real products here are not).  Where longdouble is no wider than double the products are computed
exactly with ``fractions.Fraction`` instead -- never silently in double.

The bound the tests use is derived, not measured.  A computed dot product of length L, in any order of summation, with or
without fused multiply-adds, real or complex, satisfies

    |fl(sum_j a_j x_j) - sum_j a_j x_j|  <=  gamma * sum_j |a_j| |x_j|,     gamma <= (L + 2 sqrt(2)) u / (1 - ...),

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. (3.5) for the sum and (3.13)/Lemma 3.5 for the
complex product, whose relative error is at most sqrt(2) gamma_2), so ``2 (L + 3) u * absrow`` with u = 2^-53 holds with
a factor of two to spare; the reference's own error, (L + 3) 2^-64 * absrow, is 2^-11 of that.  ``bound`` returns it per
output component: one wrong lane sum in one row is far outside it.
"""

from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0**-53
WIDE = np.finfo(LD).nmant >= 63  # x87 extended or wider; otherwise the Fraction forms run


def bound(lengths, absrow):
    """``2 (L_i + 3) u absrow_i`` as float64 (rounded up by one part in 2^52: the comparison itself must not cut it short)."""
    b = 2.0 * (np.asarray(lengths, dtype=np.float64) + 3.0) * U * np.asarray(absrow, dtype=np.float64)
    return b * (1.0 + 2.0**-50)


def _parts(a):
    a = np.asarray(a)
    re = np.ascontiguousarray(a.real).astype(LD)
    im = np.ascontiguousarray(a.imag).astype(LD) if np.iscomplexobj(a) else None
    return re, im


def _join(re, im, cplx):
    """float64 / complex128 view of a longdouble result (for subtraction from a double result use the longdouble parts)."""
    return (re.astype(np.float64) + 1j * im.astype(np.float64)) if cplx else re.astype(np.float64)


class ExtResult:
    """A product in extended precision: ``re``/``im`` longdouble parts (``im`` None for real results), ``absrow`` = sum of the
    moduli of the terms of every component, ``lengths`` = the number of terms."""

    def __init__(self, re, im, absrow, lengths):
        self.re, self.im, self.absrow, self.lengths = re, im, absrow, lengths

    @property
    def is_complex(self):
        return self.im is not None

    def value(self):
        return _join(self.re, self.im, self.is_complex)

    def error(self, got):
        """|got - ref| per component, the difference taken in longdouble."""
        got = np.asarray(got)
        dr = np.ascontiguousarray(got.real).astype(LD) - self.re
        if self.is_complex:
            di = np.ascontiguousarray(got.imag).astype(LD) - self.im
            return np.hypot(dr, di).astype(np.float64)
        assert not np.iscomplexobj(got)
        return np.abs(dr).astype(np.float64)

    def bound(self):
        return bound(self.lengths, self.absrow)


def _frac_terms(ar, ai, xr, xi):
    """exact real and imaginary parts of a x (Fractions)"""
    ar, ai, xr, xi = (Fraction(float(t)) for t in (ar, ai, xr, xi))
    return ar * xr - ai * xi, ar * xi + ai * xr


def spmv_ext(A, x, trans=None, force_fraction=False):
    """``A x`` (``trans`` None), ``A^T x`` ("T") or ``A^H x`` ("H") for a scipy CSR matrix, entry by entry in longdouble.

    Works on the stored entries as they are: duplicates, explicit zeros and unsorted rows included.  Returns an
    :class:`ExtResult`; a component without entries is exactly 0 with length 0."""
    import scipy.sparse as sp

    assert sp.isspmatrix_csr(A) and trans in (None, "T", "H")
    n, nc = A.shape
    x = np.asarray(x)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = np.asarray(A.indices, dtype=np.int64)
    out_idx, in_idx, nout = (rows, cols, n) if trans is None else (cols, rows, nc)
    assert x.shape == ((nc,) if trans is None else (n,))
    cplx = np.iscomplexobj(A.data) or np.iscomplexobj(x)
    lengths = np.bincount(out_idx, minlength=nout).astype(np.int64)
    ar, ai = _parts(A.data)
    xr, xi = _parts(x)
    if ai is None:
        ai = np.zeros_like(ar)
    if xi is None:
        xi = np.zeros_like(xr)
    if trans == "H":
        ai = -ai
    xr, xi = xr[in_idx], xi[in_idx]
    absterm = np.hypot(ar, ai) * np.hypot(xr, xi)
    absrow = np.zeros(nout, dtype=LD)
    np.add.at(absrow, out_idx, absterm)
    re, im = np.zeros(nout, dtype=LD), np.zeros(nout, dtype=LD)
    if WIDE and not force_fraction:
        # the four real products are rounded once each in longdouble, then summed in storage order
        np.add.at(re, out_idx, ar * xr)
        np.add.at(re, out_idx, -(ai * xi))
        np.add.at(im, out_idx, ar * xi)
        np.add.at(im, out_idx, ai * xr)
    else:
        fr = [Fraction(0)] * nout
        fi = [Fraction(0)] * nout
        for p, o in enumerate(out_idx):
            tr, ti = _frac_terms(ar[p], ai[p], xr[p], xi[p])
            fr[o] += tr
            fi[o] += ti
        re = np.array([LD(float(f)) for f in fr], dtype=LD)  # exact sum, rounded once to double
        im = np.array([LD(float(f)) for f in fi], dtype=LD)
    return ExtResult(re, im if cplx else None, absrow, lengths)


_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max(1, min(4, os.cpu_count() or 1)))
    return _POOL


def _ld_matmul(A, B):
    """real longdouble ``A @ B`` (``np.dot``: twice as fast as the matmul loops for this type), the rows of A dealt to a few
    threads -- numpy has no BLAS for longdouble and the loops release the interpreter lock.  Every entry is one sequential
    dot product whichever thread computes it."""
    nt = _pool()._max_workers
    if nt == 1 or A.shape[0] < 4 * nt or A.shape[0] * A.shape[1] * B.shape[1] < 1 << 21:
        return np.dot(A, B)
    cuts = np.linspace(0, A.shape[0], nt + 1).astype(int)
    parts = list(_pool().map(lambda s: np.dot(A[cuts[s] : cuts[s + 1]], B), range(nt)))
    return np.concatenate(parts, axis=0)


def _cmatmul(Ar, Ai, Br, Bi):
    """(Ar + i Ai)(Br + i Bi) in longdouble parts; a None imaginary part is zero"""
    re = _ld_matmul(Ar, Br)
    im = None
    if Ai is not None and Bi is not None:
        re = re - _ld_matmul(Ai, Bi)
        im = _ld_matmul(Ar, Bi) + _ld_matmul(Ai, Br)
    elif Ai is not None:
        im = _ld_matmul(Ai, Br)
    elif Bi is not None:
        im = _ld_matmul(Ar, Bi)
    return re, im


def matmul_ext(V, Y, force_fraction=False):
    """``V @ Y`` in longdouble with ``absrow = |V| |Y|`` (moduli) and length = the inner dimension."""
    V, Y = np.asarray(V), np.asarray(Y)
    assert V.ndim == 2 and Y.ndim == 2 and V.shape[1] == Y.shape[0]
    Vr, Vi = _parts(V)
    Yr, Yi = _parts(Y)
    absV = np.hypot(Vr, Vi) if Vi is not None else np.abs(Vr)
    absY = np.hypot(Yr, Yi) if Yi is not None else np.abs(Yr)
    absrow = _ld_matmul(absV, absY)
    cplx = Vi is not None or Yi is not None
    if WIDE and not force_fraction:
        re, im = _cmatmul(Vr, Vi, Yr, Yi)
    else:
        n, m, k = V.shape[0], V.shape[1], Y.shape[1]
        zV = np.zeros_like(Vr) if Vi is None else Vi
        zY = np.zeros_like(Yr) if Yi is None else Yi
        re, im = np.zeros((n, k), dtype=LD), np.zeros((n, k), dtype=LD)
        for i in range(n):
            for c in range(k):
                sr, si = Fraction(0), Fraction(0)
                for j in range(m):
                    tr, ti = _frac_terms(Vr[i, j], zV[i, j], Yr[j, c], zY[j, c])
                    sr += tr
                    si += ti
                re[i, c], im[i, c] = LD(float(sr)), LD(float(si))
        if not cplx:
            im = None
    lengths = np.full(absrow.shape, V.shape[1], dtype=np.int64)
    return ExtResult(re, im if cplx else None, absrow, lengths)


def qr_positive_ext(X, panel=24):
    """The unique Q factor (R with a positive diagonal) of a complex n x m matrix of full column rank, in longdouble: block
    classical Gram-Schmidt, every projection applied twice (against the finished columns panel by panel, then column by
    column inside the panel).  Returns ``(Qr, Qi)``, longdouble n x m.  Loss of orthogonality of CGS2 is O(u_ld) for
    cond(X) u_ld << 1, i.e. 2^-11 of what double arithmetic can reach."""
    if not WIDE:
        raise RuntimeError("qr_positive_ext needs a longdouble wider than double (np.finfo(np.longdouble).nmant >= 63)")
    X = np.asarray(X, dtype=np.complex128)
    n, m = X.shape
    Qr, Qi = _parts(X)
    for p0 in range(0, m, panel):
        p1 = min(p0 + panel, m)
        Pr, Pi = Qr[:, p0:p1].copy(), Qi[:, p0:p1].copy()
        if p0 > 0:
            Br, Bi = Qr[:, :p0], Qi[:, :p0]
            BrT, BiT = np.ascontiguousarray(Br.T), np.ascontiguousarray(Bi.T)
            for _ in range(2):
                Cr, Ci = _cmatmul(BrT, -BiT, Pr, Pi)  # Q^H P
                Dr, Di = _cmatmul(Br, Bi, Cr, Ci)
                Pr -= Dr
                Pi -= Di
        for c in range(p1 - p0):
            wr, wi = Pr[:, c].copy(), Pi[:, c].copy()
            if c > 0:
                Sr, Si = Pr[:, :c], Pi[:, :c]
                for _ in range(2):
                    cr = np.dot(wr, Sr) + np.dot(wi, Si)  # conj(S)^T w
                    ci = np.dot(wi, Sr) - np.dot(wr, Si)
                    wr -= np.dot(Sr, cr) - np.dot(Si, ci)
                    wi -= np.dot(Sr, ci) + np.dot(Si, cr)
            nrm = np.sqrt(np.dot(wr, wr) + np.dot(wi, wi))
            assert nrm > 0
            Pr[:, c], Pi[:, c] = wr / nrm, wi / nrm
        Qr[:, p0:p1], Qi[:, p0:p1] = Pr, Pi
    return Qr, Qi


def gram_defect_ext(V):
    """max |V^H V - I| with the Gram matrix formed in longdouble (V complex double, n x m)."""
    Vr, Vi = _parts(np.asarray(V, dtype=np.complex128))
    VrT, ViT = np.ascontiguousarray(Vr.T), np.ascontiguousarray(Vi.T)
    Gr, Gi = _cmatmul(VrT, -ViT, Vr, Vi)
    Gr = Gr - np.eye(V.shape[1], dtype=LD)
    return float(np.max(np.hypot(Gr, Gi)))
