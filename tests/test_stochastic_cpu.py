"""CPU suite: stochastic forcing (``Solver.stochastic``, ``tests/stochastic_reference.py``).  The definition of the quadrature operator
against a Lyapunov solve, the numpy restatement of the library's iteration against the dense eigenvalues of S2k
(``tests/golden/stochastic_s2k.json``), the operator's symmetries, and what the front end refuses before it touches a device."""

import json
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import stochastic_reference as ref
from Solver.stochastic import StochasticConfig, StochasticForcingSolver, gauss_legendre_band, plan_factor_sets, quadrature, tan_rule

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "stochastic_s2k.json").read_text())


def leading(S, k=4):
    return np.sort(np.linalg.eigvals(S).real)[::-1][:k]


def test_quadrature_rules_are_those_of_the_reference():
    for got, want in ((gauss_legendre_band(0.0, 1.5, 8), ref.gauss_band(0.0, 1.5, 8)), (tan_rule(0.7, 16), ref.tan_rule(0.7, 16)),
                      (quadrature(8, band=(0.0, 1.5)), ref.gauss_band(0.0, 1.5, 8)), (quadrature(16, band=(0.0, np.inf), scale=0.7), ref.tan_rule(0.7, 16))):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    om, w = quadrature(3, omegas=[0.1, 0.5], weights=[0.2, 0.3])
    assert om.tolist() == [0.1, 0.5] and w.tolist() == [0.2, 0.3]
    assert np.isclose(sum(gauss_legendre_band(0.25, 1.5, 8)[1]), 1.25)
    assert GOLDEN["omegas"] == ref.gauss_band(*ref.BAND, 8)[0].tolist()


def test_tan_rule_reproduces_the_lyapunov_variances():
    """The seeded dense stable pair (n = 40, SPD M): the four largest eigenvalues of ``P M`` from
    ``scipy.linalg.solve_continuous_lyapunov`` against those of the quadrature operator under ``omega = s tan(theta)``.  64 nodes agree
    to 1e-10 relative (measured 2e-15: the margin covers BLAS differences); 16 nodes do not agree to 1e-8 (measured 1e-5), so the test
    tells a converged quadrature from one that is not."""
    A, M = ref.lyapunov_pair()
    want = ref.lyapunov_variances(A, M)
    As, Ms = sp.csr_matrix(A), sp.csr_matrix(M)
    err = {}
    for N in (16, 64):
        om, w = quadrature(N, band=(0.0, np.inf), scale=ref.LYAPUNOV_SCALE)
        err[N] = float((np.abs(leading(ref.dense_operator(As, Ms, om, w)) - want) / want).max())
    print(f"Lyapunov pair: relative error of the four largest variances {err}")
    assert err[64] <= 1e-10
    assert err[16] > 1e-8


@pytest.fixture(scope="module")
def s2k_host():
    A, M = ref.case("S2k")
    om, w = ref.gauss_band(*ref.BAND, 8)
    return ref.HostStochastic(A, M, om, w)


@pytest.fixture(scope="module")
def s2k_restated(s2k_host):
    n = s2k_host.Qq.shape[0]
    return ref.stochastic_trl(s2k_host, "eofs", 4, 24, 1e-10, np.random.default_rng(0).standard_normal(n))


def test_restated_iteration_against_the_dense_eigenvalues(s2k_restated):
    """S2k, band [0, 1.5], 8 nodes, ncv = 24, atol = 1e-10: the restated thick-restart iteration against the dense eigenvalues of the
    operator (committed: the dense solve takes 20 s), ``|theta_j - theta_j^dense| <= 1e-10 theta_1`` -- the bound of the GPU test for
    this iteration at this tolerance -- and the issue's six-decimal values as a cross-check of the definition."""
    got, dense = s2k_restated["variances"], np.array(GOLDEN["eofs"][:4])
    err = np.abs(got - dense).max() / dense[0]
    print(f"restated: variances {got}, |theta - dense|_max / theta_1 = {err:.2e}, applies {s2k_restated['applies']}, restarts {s2k_restated['restarts']}")
    assert len(got) == 4 and (np.diff(got) <= 0.0).all()
    assert err <= 1e-10
    assert np.allclose(dense, ref.VARIANCES_S2K_8, rtol=0.0, atol=1e-6)
    assert GOLDEN["eofs_max_imag"] == 0.0


def test_spectrum_rows_sum_to_the_variances(s2k_host, s2k_restated):
    """One apply per mode: the node terms ``(w_k / pi) (Q e_j)^T Re W_k e_j`` sum to ``theta_j`` (1e-8 relative: the modes are
    converged to 1e-10 and the Rayleigh quotient of a self-adjoint operator is second order in the mode's error), and the modes are
    orthonormal in the weight."""
    X, theta = s2k_restated["modes"], s2k_restated["variances"]
    assert np.abs(X.T @ (s2k_host.Qq @ X) - np.eye(4)).max() <= 1e-10
    for j in range(4):
        terms = s2k_host.apply(X[:, j], "eofs")[1]
        assert terms.shape == (8,) and abs(terms.sum() - theta[j]) <= 1e-8 * theta[j]


@pytest.mark.parametrize("kind", ["eofs", "optimals"])
def test_both_kinds_are_self_adjoint_in_their_weight(kind):
    """On the dense pair with a forcing and a response window: ``Q S`` is symmetric to rounding (1e-12 relative in the Frobenius norm:
    the dense solves are backward stable and the nodes' matrices have condition numbers below 100), its eigenvalues are real and
    non-negative, and the operator applied through SuperLU factors per node is the dense one."""
    A, M = ref.lyapunov_pair()
    n = A.shape[0]
    d1, d2 = (np.arange(n) < 25).astype(float), (np.arange(n) >= 10).astype(float)
    Qf, Qq = d1[:, None] * M * d1[None, :], d2[:, None] * M * d2[None, :]
    om, w = ref.tan_rule(ref.LYAPUNOV_SCALE, 16)
    S = ref.dense_operator(sp.csr_matrix(A), sp.csr_matrix(M), om, w, Qf, Qq, kind=kind)
    Q = Qq if kind == "eofs" else Qf
    QS = Q @ S
    assert np.linalg.norm(QS - QS.T) <= 1e-12 * np.linalg.norm(QS)
    ev = np.linalg.eigvals(S)
    assert np.abs(ev.imag).max() <= 1e-10 * np.abs(ev).max() and ev.real.min() >= -1e-12 * np.abs(ev).max()
    host = ref.HostStochastic(sp.csr_matrix(A), sp.csr_matrix(M), om, w, sp.csr_matrix(Qf), sp.csr_matrix(Qq))
    v = np.random.default_rng(1).standard_normal(n)
    y, terms = host.apply(v, kind)
    assert np.linalg.norm(y - S @ v) <= 1e-12 * np.linalg.norm(S @ v)
    assert abs(terms.sum() - v @ (Q @ (S @ v))) <= 1e-12 * abs(v @ (Q @ (S @ v)))


def test_kinds_share_their_trace():
    """``tr S = tr S'`` (cyclic permutations under the trace), although the spectra differ: a check of the golden file's two kinds."""
    assert abs(GOLDEN["eofs_trace"] - GOLDEN["optimals_trace"]) <= 1e-9 * GOLDEN["eofs_trace"]
    assert abs(GOLDEN["eofs"][0] - GOLDEN["optimals"][0]) > 1e-6 * GOLDEN["eofs"][0]


def test_planner_refuses_with_both_figures():
    assert plan_factor_sets(8, 100, 1001) == 800
    with pytest.raises(MemoryError) as info:
        plan_factor_sets(16, 1_000_000, 10_000_000)
    text = str(info.value)
    assert "16000000" in text and "8000000" in text and "at most 8 nodes" in text
    assert plan_factor_sets(16, 1_000_000, 20_000_000) == 16_000_000


def test_quadrature_refusals():
    for kw in (dict(), dict(band=(0.0, 1.0), omegas=[0.1], weights=[1.0]), dict(omegas=[0.1]), dict(band=(1.0, 0.5)), dict(band=(-0.1, 0.5)),
               dict(band=(0.0, np.inf)), dict(band=(0.5, np.inf), scale=1.0), dict(band=(0.0, 1.0), scale=1.0), dict(band=(0.0, np.inf), scale=-1.0),
               dict(omegas=[0.1, 0.2], weights=[1.0]), dict(omegas=[-0.1], weights=[1.0]), dict(omegas=[0.1], weights=[-1.0]),
               dict(omegas=[0.1], weights=[0.0]), dict(omegas=[np.nan], weights=[1.0])):
        with pytest.raises(ValueError):
            quadrature(4, **kw)
    with pytest.raises(ValueError, match="nodes"):
        quadrature(0, band=(0.0, 1.0))


def test_front_end_refusals_need_no_device():
    A, M = ref.case("S2k")
    n = A.shape[0]
    with pytest.raises(ValueError, match="real A"):
        StochasticForcingSolver(A.astype(np.complex128), M)
    with pytest.raises(ValueError, match="real M"):
        StochasticForcingSolver(A, M.astype(np.complex128))
    with pytest.raises(ValueError, match="needs M"):
        StochasticForcingSolver(A, None)
    skew = M + sp.csr_matrix(([1.0], ([0], [5])), shape=M.shape)
    with pytest.raises(ValueError, match="symmetric M"):
        StochasticForcingSolver(A, skew)
    with pytest.raises(ValueError, match="not both"):
        StochasticForcingSolver(A, M, response_window=np.ones(n), response_weight=M)
    with pytest.raises(ValueError, match="ncv"):
        StochasticForcingSolver(A, M, StochasticConfig(num_modes=4, ncv=4))
    with pytest.raises(ValueError, match="nodes"):
        StochasticForcingSolver(A, M, StochasticConfig(nodes=0))
    with pytest.raises(ValueError, match="discount"):
        StochasticForcingSolver(A, M, discount=1j)
    with pytest.raises(NotImplementedError, match="one GPU"):
        StochasticForcingSolver(A, M, layout="sharded")
    sf = StochasticForcingSolver(A, M)
    assert sf.config == StochasticConfig(num_modes=4, ncv=24, atol=1e-8, max_it=500, nodes=16)
    with pytest.raises(ValueError, match="kind"):
        sf.solve(band=(0.0, 1.5), kind="modes")
    with pytest.raises(ValueError):
        sf.solve()


def test_docstrings_state_what_is_computed():
    import Solver.stochastic as mod

    for text in (mod.__doc__, StochasticForcingSolver.__doc__):
        assert "quadrature operator" in text and "discount" in text
    assert "caller's to check" in mod.__doc__
