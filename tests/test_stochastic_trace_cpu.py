"""CPU suite: the trace of the stochastic-forcing operator by block probes -- the two-column estimator's definition on a dense pair,
the host summaries of ``Solver.stochastic``, the numpy restatement of the probe generator, and the argument checks of the front end
(none of which needs a device)."""

import math

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import stochastic_reference as ref
import trace_reference as tref
from Solver.stochastic import StochasticForcingSolver, TraceConfig, captured_fractions, trace_summary


def lyapunov_host():
    A, M = ref.lyapunov_pair(40)
    om, w = ref.tan_rule(ref.LYAPUNOV_SCALE, 32)
    return A, M, om, w, ref.HostStochastic(sp.csr_matrix(A), sp.csr_matrix(M), om, w)


@pytest.fixture(scope="module")
def lyapunov():
    return lyapunov_host()


@pytest.mark.parametrize("kind", ["eofs", "optimals"])
def test_unit_vectors_give_the_trace(lyapunov, kind):
    """Summed over the 40 unit vectors the two-column form is ``tr S`` of the dense operator (1e-12 relative: both are sums of the
    same 40 x 32 solves) and, the tan rule resolving the integral, ``tr(P M)`` of the Lyapunov solve (1e-8)."""
    from scipy.linalg import solve_continuous_lyapunov

    A, M, om, w, host = lyapunov
    S = ref.dense_operator(sp.csr_matrix(A), sp.csr_matrix(M), om, w, kind=kind)
    total = tref.forms(host, np.eye(40), kind).sum()
    print(f"{kind}: two-column sum {total!r}, dense trace {np.trace(S)!r}")
    assert abs(total - np.trace(S)) <= 1e-12 * abs(np.trace(S))
    Minv = np.linalg.inv(M)
    P = solve_continuous_lyapunov(Minv @ A, -Minv)
    assert abs(total - np.trace(P @ M)) <= 1e-8 * np.trace(P @ M)


@pytest.mark.parametrize("kind", ["eofs", "optimals"])
def test_deflated_unit_vectors_give_the_remainder(lyapunov, kind):
    """Deflated by the 4 leading dense eigenvectors (orthonormal in the kind's weight), the sum is ``tr S - sum(theta)``."""
    A, M, om, w, host = lyapunov
    S = ref.dense_operator(sp.csr_matrix(A), sp.csr_matrix(M), om, w, kind=kind)
    Q = host.weight(kind).toarray()
    theta, V = np.linalg.eig(S)
    order = np.argsort(-theta.real)[:4]
    U = V[:, order].real
    U = U / np.sqrt(np.einsum("ij,ij->j", U, Q @ U))
    assert np.abs(U.T @ Q @ U - np.eye(4)).max() <= 1e-10  # (distinct eigenvalues of an operator self-adjoint in Q)
    rest = tref.forms(host, np.eye(40), kind, U).sum()
    want = np.trace(S) - theta.real[order].sum()
    print(f"{kind}: deflated sum {rest!r}, tr S - sum theta {want!r}")
    assert abs(rest - want) <= 1e-12 * abs(np.trace(S))
    # ... and the one-column form of the operator itself agrees term by term
    Z = np.random.default_rng(1).standard_normal((40, 3))
    a, b = tref.node_terms(host, Z, kind, U), tref.one_column_terms(host, Z, kind, U)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).sum(axis=0).max()


def test_trace_summary_known_answers():
    s = trace_summary([1.0, 2.0, 3.0, 6.0], [10.0, 5.0])
    assert s["total"] == 15.0 + 3.0 and s["remainder"] == 3.0 and not s["exact"]
    # the sample variance with ddof = 1 of (1, 2, 3, 6) is (4 + 1 + 0 + 9) / 3
    assert s["stderr"] == pytest.approx(math.sqrt(14.0 / 3.0) / 2.0, rel=1e-15)
    s = trace_summary([4.0])
    assert s["total"] == 4.0 and math.isnan(s["stderr"])
    s = trace_summary([1.0, 2.0, 3.0], [7.0], exact=True)
    assert s["total"] == 13.0 and s["stderr"] == 0.0 and s["exact"]
    s = trace_summary(np.array([2.0, 4.0]))
    assert s["total"] == 3.0 and s["stderr"] == pytest.approx(1.0)
    with pytest.raises(ValueError):
        trace_summary([])


def test_captured_fractions_known_answers():
    frac, err = captured_fractions([4.0, 2.0, 1.0], 10.0, 0.5)
    assert np.array_equal(frac, [0.4, 0.6, 0.7])
    assert np.allclose(err, np.array([0.4, 0.6, 0.7]) * 0.05, rtol=1e-15)
    assert (np.diff(frac) > 0).all()
    frac, err = captured_fractions(ref.VARIANCES_S2K_8, 25411.73396, 0.0)
    assert (np.diff(frac) > 0).all() and (err == 0.0).all()
    assert round(float(frac[-1]), 6) == 0.064297
    with pytest.raises(ValueError):
        captured_fractions([1.0], 0.0)


def test_generator_is_a_function_of_seed_probe_and_row():
    n = 1953
    Z = tref.probes(n, 64, seed=0)
    assert set(np.unique(Z)) == {-1.0, 1.0}
    # however the probes are grouped: one by one, in blocks, out of order
    assert np.array_equal(Z[:, 5:9], tref.probe_columns(n, [5, 6, 7, 8], 0))
    assert np.array_equal(Z[:, [40, 3]], np.column_stack([tref.probe_columns(n, [40], 0)[:, 0], tref.probe_columns(n, [3], 0)[:, 0]]))
    assert np.array_equal(Z[:100], tref.probes(100, 64, 0))  # (a row's entry does not depend on n)
    # different probe indices and different seeds give different columns
    assert len({Z[:, p].tobytes() for p in range(64)}) == 64
    assert not np.array_equal(Z[:, 0], tref.probes(n, 1, seed=1)[:, 0])
    # the share of +1 over 64 x 1953 entries: 0.5 +- 0.005 is 3.5 sigma of the binomial (sigma = 0.5 / sqrt(124992) = 0.0014)
    share = float((Z > 0).mean())
    print(f"share of +1: {share:.5f}")
    assert abs(share - 0.5) <= 0.005
    # columns are not correlated beyond chance: |z_p . z_q| / n stays below 5 / sqrt(n) for all 2016 pairs (5 sigma)
    G = Z.T @ Z / n - np.eye(64)
    assert np.abs(G).max() <= 5.0 / math.sqrt(n)


def test_trace_arguments_are_checked_without_a_device():
    A, M = ref.case("S2k")
    n = A.shape[0]
    sf = StochasticForcingSolver(A, M)
    for bad in (0, -3, TraceConfig(probes=0), TraceConfig(probes=-1), np.ones((n + 1, 2)), np.ones(n), np.ones((n, 0)), TraceConfig(probes=4, batch=-1),
                np.ones((n, 2), dtype=complex)):
        with pytest.raises(ValueError, match="trace"):
            sf.solve(band=(0.0, 1.5), trace=bad)
    for bad in (0, -3, np.ones((n + 1, 2)), np.ones(n)):
        with pytest.raises(ValueError, match="trace"):
            sf.total_variance(band=(0.0, 1.5), probes=bad)
    with pytest.raises(ValueError, match="kind"):
        sf.total_variance(band=(0.0, 1.5), kind="modes")
    assert TraceConfig() == TraceConfig(probes=32, seed=0, deflate=True, batch=0)
