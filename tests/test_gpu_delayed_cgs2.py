"""GPU suite: the delayed-reorthogonalisation Arnoldi step (DCGS2) of the pipelined path (``csrc/blas.hip``: ``dcgs_dot_kernel``,
``dcgs_update_kernel``, ``cgs_tail_kernel<.., true>``; ``csrc/solver.hip``: ``krylov_enqueue_dstep``, ``lsa_krylov_extend``)
against numpy, and against the five-launch CGS2 it replaces (``LSA_KRYLOV_DELAYED=0``, read once per process: child
processes)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = str(Path(__file__).resolve().parents[1])


def _numpy_dcgs2(Q, p, y, first):
    """One step: (q, w, column of H before the host's H a term, nu) -- the kernels' arithmetic in numpy."""
    j = Q.shape[1]
    b, beta = Q.conj().T @ y, np.vdot(p, y)
    if first:
        q, nu, c, a = p, 1.0, beta, np.zeros(j, dtype=complex)
    else:
        a = Q.conj().T @ p
        nu = np.sqrt(np.vdot(p, p).real - np.vdot(a, a).real)
        q = (p - Q @ a) / nu
        c = (beta - np.vdot(a, b)) / nu
    w = (y - Q @ b - c * q) / nu
    return q, w, a, b, c, nu


@pytest.mark.parametrize("j", [1, 7, 8, 79, 125])
def test_reduce_and_update_against_numpy(hip_ctx, j):
    """n = 30 876 rows (31 row chunks, the last one ragged; a ragged last workgroup of the update), OP = (D - sigma I)^-1 with D
    diagonal, which numpy applies to rounding: extend(j, j + 2) from an orthonormal V[:, 0:j+1] runs the first step of a call
    (V[:, j] final), one step with a pending vector and the flush.  V and the two new columns of H against numpy to 1e-13."""
    import lsa_hip

    n, ncv, sigma = 30876, 127, 0.37 + 0.11j
    d = np.linspace(1.0, 4.0, n) + 0.05j * np.cos(np.arange(n))
    D = sp.diags(d).tocsr()
    op = lsa_hip.ShiftInvertOperator(hip_ctx, lsa_hip.CsrMatrix.from_scipy(hip_ctx, D), lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.identity(n, format="csr")),
                                     sigma, pc_type=2)
    kb = lsa_hip.KrylovBasis(hip_ctx, op, ncv)
    rng = np.random.default_rng(j)
    for c in range(j + 1):
        kb.inject(c, rng.standard_normal(n) + 1j * rng.standard_normal(n))
    V0 = kb.ritz_vectors(j + 1, np.eye(j + 1, dtype=complex), False)
    H = np.zeros((ncv + 1, ncv), dtype=np.complex128, order="F")
    Hs = np.triu(rng.standard_normal((j + 1, j)) + 1j * rng.standard_normal((j + 1, j)), -1)  # stands for the caller's columns
    H[: j + 1, :j] = Hs
    assert kb.extend(j, j + 2, H) == -1
    V1 = kb.ritz_vectors(j + 3, np.eye(j + 3, dtype=complex), False)
    opx = lambda x: x / (d - sigma)  # noqa: E731

    Q, p = V0[:, :j], V0[:, j]
    q0, w0, _, b0, c0, _ = _numpy_dcgs2(Q, p, opx(p), True)
    Q1 = np.column_stack([Q, q0])
    q1, w1, a1, b1, c1, nu1 = _numpy_dcgs2(Q1, w0, opx(w0), False)
    Q2 = np.column_stack([Q1, q1])
    a2 = Q2.conj().T @ w1
    nu2 = np.sqrt(np.vdot(w1, w1).real - np.vdot(a2, a2).real)
    q2 = (w1 - Q2 @ a2) / nu2

    Hn = H.copy()
    Hn[:, j:] = 0
    Hn[: j + 1, j] = np.append(b0, c0) + a1
    Hn[j + 1, j] = nu1
    Hn[: j + 2, j + 1] = (np.append(b1, c1) - Hn[: j + 2, : j + 1] @ a1) / nu1 + a2
    Hn[j + 2, j + 1] = nu2
    assert np.abs(V1[:, : j + 1] - V0).max() <= 1e-13
    assert np.abs(V1[:, j + 1] - q1).max() <= 1e-13 * np.abs(q1).max()
    assert np.abs(V1[:, j + 2] - q2).max() <= 1e-13 * np.abs(q2).max()
    assert np.abs(H - Hn).max() <= 1e-13 * np.abs(Hn[:, j:]).max()


def test_basis_after_one_extend_is_orthonormal_and_satisfies_the_arnoldi_relation(hip_ctx):
    """S30k, extend(0, 80) in one call (batches of 16, a flush at the end): max |V^H V - I| <= 1e-13 and
    ||OP V_80 - V_81 H|| / ||H|| <= 1e-12, OP applied on the device."""
    import lsa_hip
    from synthetic import fem

    es = fem.cylinder_case("S30k")
    op = lsa_hip.ShiftInvertOperator(hip_ctx, lsa_hip.CsrMatrix.from_scipy(hip_ctx, es.A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, es.M), fem.SIGMA_RE50,
                                     pc_type=2)
    kb = lsa_hip.KrylovBasis(hip_ctx, op, 80)
    kb.inject(0, np.random.default_rng(5).standard_normal(es.n) + 0j)
    H = np.zeros((81, 80), dtype=np.complex128, order="F")
    assert kb.extend(0, 80, H) == -1
    V = kb.ritz_vectors(81, np.eye(81, dtype=complex), False)
    assert np.abs(V.conj().T @ V - np.eye(81)).max() <= 1e-13
    x, y = lsa_hip.DeviceVector(hip_ctx, es.n), lsa_hip.DeviceVector(hip_ctx, es.n)
    OPV = np.empty((es.n, 80), dtype=complex)
    for c in range(80):
        x.upload(np.ascontiguousarray(V[:, c]))
        op.apply(x, y)
        OPV[:, c] = y.numpy()
    assert np.linalg.norm(OPV - V @ H) / np.linalg.norm(H) <= 1e-12


_BENCH_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd"]
from synthetic import fem
from Solver.eigen import EigenSolver, EigensolverConfig
from Solver.utils import PreconditionerType, iSTType
es = fem.cylinder_case("S30k")
s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=20, atol=1e-10, ncv=80), check_hermitian=False)
s.solver.set_st_type(iSTType.SINVERT); s.solver.set_st_pc_type(PreconditionerType.LU); s.solver.set_target(fem.SIGMA_RE50)
pairs = s.solve()
print(json.dumps({"lam": [[p[0].real, p[0].imag] for p in pairs[:20]], "applies": s.solver.stats["op_applies"], "n": len(pairs)}))
"""


def test_bench_configuration_with_and_without_the_delayed_form():
    """The bench configuration (S30k, 20 pairs, ncv = 80) with LSA_KRYLOV_DELAYED=0 (five-launch CGS2) and =1: 20 pairs each,
    the same operator applies, the eigenvalues to 1e-11 relative."""
    runs = {}
    for knob in ("0", "1"):
        p = subprocess.run([sys.executable, "-c", _BENCH_CHILD, ROOT], env={**os.environ, "LSA_KRYLOV_DELAYED": knob}, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        runs[knob] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert runs["0"]["n"] >= 20 and runs["1"]["n"] >= 20
    assert runs["0"]["applies"] == runs["1"]["applies"]
    lam0 = np.array([complex(a, b) for a, b in runs["0"]["lam"]])
    lam1 = np.array([complex(a, b) for a, b in runs["1"]["lam"]])
    assert np.max(np.abs(lam1 - lam0) / np.abs(lam0)) <= 1e-11
