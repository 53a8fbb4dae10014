"""CPU restatement of the delayed-reorthogonalisation Arnoldi step (DCGS2) of the pipelined path (``csrc/solver.hip``,
``krylov_enqueue_dstep`` / ``lsa_krylov_extend``; kernels ``dcgs_dot_kernel`` / ``dcgs_update_kernel`` in ``csrc/blas.hip``):
the same recurrence, host algebra, flush and breakdown rules in numpy, driven by the product's Krylov-Schur driver on the
oracle's SuperLU shift-invert, against the CGS2 test double of ``tests/helpers.py``."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers
from synthetic import fem


class DelayedKrylovBackend(helpers.NumpyKrylovBackend):
    """On entry to step j (except the first of an ``extend`` call) V[:, j] is the previous step's vector projected once and
    not normalised, and column j - 1 of H is provisional.  One reduction (a = Q^H p, alpha = p^H p, b = Q^H y, beta = p^H y)
    and one update per step; the flush at the end of a call makes V[:, j1] and column j1 - 1 final."""

    def _second_pass(self, j, H):
        """a, nu of p = V[:, j] against Q = V[:, :j]: V[:, j] final, column j - 1 of H final.  Returns (a, nu, broke_down)."""
        Q, p = self.V[:, :j], self.V[:, j]
        a = Q.conj().T @ p
        nu = np.sqrt(max(np.vdot(p, p).real - np.vdot(a, a).real, 0.0))
        self.V[:, j] = (p - Q @ a) / nu if nu > 0 else 0.0
        H[:j, j - 1] += a
        H[j, j - 1] = nu
        return a, nu, nu <= 1e-14 * max(np.abs(H[:j, j - 1]).max(), 1e-300)

    def extend(self, j0, j1, H):
        pending = False
        for j in range(j0, j1):
            Q = self.V[:, :j]
            y = self.op(self.V[:, j])  # OP p, p unnormalised
            b, beta = Q.conj().T @ y, np.vdot(self.V[:, j], y)
            if pending:
                a, nu, broke = self._second_pass(j, H)
                if broke:
                    return j - 1
                c = (beta - np.vdot(a, b)) / nu
                h = (np.append(b, c) - H[: j + 1, :j] @ a) / nu
            else:
                nu, c = 1.0, beta
                h = np.append(b, c)
            self.applies += 1
            w = (y - Q @ b - c * self.V[:, j]) / nu
            self.V[:, j + 1] = w
            H[:, j] = 0
            H[: j + 1, j] = h
            H[j + 1, j] = np.linalg.norm(w)
            pending = True
            if H[j + 1, j].real <= 1e-14 * max(np.abs(h).max(), 1e-300):
                return j
        if pending:
            if self._second_pass(j1, H)[2]:
                return j1 - 1
        return -1


def _solve(case, cls):
    from lsa_hip.krylov_schur import krylov_schur

    es = fem.cylinder_case(case)
    sigma = fem.SIGMA_RE50
    lu = spla.splu((es.A - sigma * es.M).tocsc())
    be = cls(lambda x: lu.solve(es.M @ x), es.n, 80)
    res = krylov_schur(be, 20, 1e-10, 200, lambda th: -np.abs(th))
    return res, be


@pytest.fixture(scope="module")
def s5k_runs():
    return {cls.__name__: _solve("S5k", cls) for cls in (helpers.NumpyKrylovBackend, DelayedKrylovBackend)}


def test_delayed_cgs2_matches_cgs2_on_the_bench_settings(s5k_runs):
    """S5k, k = 20, ncv = 80, tol 1e-10: the same operator applies and restarts, the eigenvalues to 1e-12, an orthonormal
    basis to 1e-13."""
    (r0, _), (r1, be) = s5k_runs["NumpyKrylovBackend"], s5k_runs["DelayedKrylovBackend"]
    assert r1.nconv >= 20 and r0.nconv == r1.nconv
    assert r1.op_applies == r0.op_applies == be.applies and r1.restarts == r0.restarts
    lam0, lam1 = fem.SIGMA_RE50 + 1.0 / r0.theta, fem.SIGMA_RE50 + 1.0 / r1.theta
    assert np.max(np.abs(lam1 - lam0) / np.abs(lam0)) <= 1e-12
    V = be.V
    assert np.abs(V.conj().T @ V - np.eye(V.shape[1])).max() <= 1e-13


def test_delayed_cgs2_arnoldi_relation_after_one_extend():
    """One call extend(0, 40) from a random start: after the flush OP V_40 = V_41 H to rounding and H Hessenberg, as CGS2."""
    es = fem.cylinder_case("S2k")
    lu = spla.splu((es.A - fem.SIGMA_RE50 * es.M).tocsc())
    op = lambda x: lu.solve(es.M @ x)  # noqa: E731
    v0 = np.random.default_rng(1).standard_normal(es.n) + 0j
    out = {}
    for cls in (helpers.NumpyKrylovBackend, DelayedKrylovBackend):
        be = cls(op, es.n, 40)
        be.inject(0, v0)
        H = np.zeros((41, 40), dtype=np.complex128, order="F")
        assert be.extend(0, 17, H) == -1 and be.extend(17, 40, H) == -1  # two calls: a flush in between
        OPV = np.column_stack([op(be.V[:, c]) for c in range(40)])
        assert np.linalg.norm(OPV - be.V @ H) / np.linalg.norm(H) <= 1e-12
        assert np.abs(be.V.conj().T @ be.V - np.eye(41)).max() <= 1e-13
        assert np.all(np.tril(H, -2) == 0)
        out[cls] = H
    Hc, Hd = out.values()
    assert np.abs(Hd - Hc).max() <= 1e-11 * np.abs(Hc).max()


def test_delayed_cgs2_reports_a_breakdown_at_its_step():
    """The start vector spans a 3-dimensional invariant subspace of a diagonal pair: the third step breaks down (judged on
    the provisional norm), after three applies, as with CGS2."""
    n = 64
    D = sp.diags(np.arange(1.0, n + 1)).tocsc()
    lu = spla.splu((D - 0.5 * sp.identity(n, format="csc")).astype(np.complex128).tocsc())
    v = np.zeros(n, dtype=np.complex128)
    v[[4, 9, 20]] = 1.0
    for cls in (helpers.NumpyKrylovBackend, DelayedKrylovBackend):
        be = cls(lu.solve, n, 12)
        be.inject(0, v)
        H = np.zeros((13, 12), dtype=np.complex128, order="F")
        assert be.extend(0, 12, H) == 2 and be.applies == 3, cls.__name__
