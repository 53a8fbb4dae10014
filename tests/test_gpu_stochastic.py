"""GPU suite: stochastic forcing (``csrc/stochastic.hip``, ``lsa_stochastic_*``, ``Solver.stochastic``) on the synthetic cylinder case
S2k (n = 1953: no multiple of 256 or 512, the last chunk of every reduction is partial; the smallest case with a real elimination
forest), against a long-double product, SuperLU on the host and the dense eigenvalues of ``tests/golden/stochastic_s2k.json``."""

import json
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401
import stochastic_reference as ref
import weighted_reference as wref
from test_lanczos_cpu import on_shared_pattern

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "stochastic_s2k.json").read_text())
U = 2.0**-53  # the unit roundoff of float64


def random_pair(seed=3):
    """Two real matrices on one pattern, 96 x 96 (the library's matrices are square): 50 rows carry entries, the others are empty,
    one row has 80 entries (more than 64: every lane of its row group takes ten), the rest between 1 and 9."""
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


def long_double_product(A, M, z, X):
    """``(y_ref, bound)``: ``Y[:, k] = (A - z_k M) X[:, k]`` summed in long double, and ``(|A| + |z_k| |M|) |X[:, k]|``."""
    n, N = X.shape
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    a, m = A.data.astype(np.longdouble), M.data.astype(np.longdouble)
    Y = np.zeros((n, N), dtype=np.clongdouble)
    B = np.zeros((n, N), dtype=np.longdouble)
    for k in range(N):
        zr, zi = np.longdouble(z[k].real), np.longdouble(z[k].imag)
        x = X[A.indices, k]
        xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
        cr, ci = a - zr * m, -zi * m
        re, im = cr * xr - ci * xi, cr * xi + ci * xr
        yr, yi, b = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
        np.add.at(yr, rows, re)
        np.add.at(yi, rows, im)
        np.add.at(b, rows, (np.abs(a) + np.sqrt(zr * zr + zi * zi) * np.abs(m)) * np.sqrt(xr * xr + xi * xi))
        Y[:, k] = yr + 1j * yi
        B[:, k] = b
    return Y, B


@pytest.mark.parametrize("N", [1, 3, 16])
@pytest.mark.parametrize("which", ["S2k", "random"])
def test_shifted_spmm_against_long_double(hip_ctx, which, N):
    """``lsa_shifted_spmm`` componentwise against a long-double product: ``|y - y_ref| <= (len_row + 2) u (|A| + |z_k| |M|) |x|``, the
    standard bound of a sum of ``len_row`` products whose factor ``a - z_k m`` carries one rounding of its own; ``u = 2^-53``.  An empty
    row gives an exact zero."""
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k")) if which == "S2k" else random_pair()
    n = A.shape[0]
    rng = np.random.default_rng(N)
    z = rng.standard_normal(N) + 1j * rng.uniform(0.0, 1.5, N)
    X = rng.standard_normal((n, N)) + 1j * rng.standard_normal((n, N))
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    Y = lsa_hip.shifted_spmm(hip_ctx, dA, dM, z, X)
    Yref, B = long_double_product(A, M, z, X)
    lens = np.diff(A.indptr).astype(np.longdouble)[:, None]
    err = np.abs(Y.astype(np.clongdouble) - Yref)
    bound = (lens + 2) * np.longdouble(U) * B
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{which}, N = {N}: worst |y - y_ref| / bound = {worst:.3f}, rows up to {int(lens.max())} entries")
    assert (err <= bound).all()
    assert (Y[np.diff(A.indptr) == 0] == 0.0).all()


def s2k_device(hip_ctx):
    import lsa_hip

    A, M = on_shared_pattern(*ref.case("S2k"))
    return A, M, lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("kind", ["eofs", "optimals"])
def test_apply_against_the_host_reference(hip_ctx, kind, windowed):
    """``lsa_stochastic_apply`` with N = 4 Gauss nodes on [0, 1.5], ``ksp_rtol = 1e-12``, against the operator applied through SuperLU
    factors per node, in the norm of the kind's weight: ``||y - y_ref|| <= 1e-9 ||y_ref||`` (from the solves: two solves of relative
    residual 1e-12 per node through operators of gain below 1e3); the node terms against the reference's to the same bound."""
    import lsa_hip

    A, M, dA, dM = s2k_device(hip_ctx)
    n = A.shape[0]
    om, w = ref.gauss_band(*ref.BAND, 4)
    d = wref.window("S2k", 2.0, 30.0) if windowed else None
    Qq = wref.weighted(M, d) if windowed else None
    host = ref.HostStochastic(A, M, om, w, None, Qq)
    basis = lsa_hip.StochasticBasis(hip_ctx, dA, dM, 1j * om, w, 12, ksp_rtol=1e-12)
    dQ = dM.windowed(d) if windowed else None
    if windowed:
        basis.set_weights(None, dQ)
    basis.set_kind(0 if kind == "eofs" else 1)
    v = np.random.default_rng(5).standard_normal(n)
    y, terms = basis.apply(v)
    info = basis.info()
    del basis
    yref, tref = host.apply(v, kind)
    Q = host.weight(kind)
    err, scale = ref.weight_norm(Q, y - yref), ref.weight_norm(Q, yref)
    print(f"{kind}, window {windowed}: ||y - y_ref||_Q / ||y_ref||_Q = {err / scale:.2e}; refined {info['solver']['refined_solves']}, "
          f"max rel res {info['solver']['max_rel_res']:.1e}")
    assert err <= 1e-9 * scale
    assert np.abs(terms - tref).max() <= 1e-9 * np.abs(tref).sum()
    assert info["solver"]["op_applies"] == 8 and info["nodes"] == 4


_SOLVED = {}


def solved(kind="eofs", nodes=8, ncv=24, num_modes=4, atol=1e-10, batch_forward=False, refine=False, tag=0):
    """One front-end solve per configuration and process: S2k, band [0, 1.5]."""
    key = (kind, nodes, ncv, num_modes, atol, batch_forward, refine, tag)
    if key not in _SOLVED:
        from Solver.stochastic import StochasticConfig, StochasticForcingSolver

        A, M = ref.case("S2k")
        sf = StochasticForcingSolver(A, M, StochasticConfig(num_modes=num_modes, ncv=ncv, atol=atol, nodes=nodes), batch_forward=batch_forward)
        sf._force_refinement = refine
        _SOLVED[key] = sf.solve(band=ref.BAND, kind=kind)
        sf.release()
    return _SOLVED[key]


@pytest.fixture(scope="module")
def s2k_host():
    A, M = ref.case("S2k")
    return ref.HostStochastic(A, M, *ref.gauss_band(*ref.BAND, 8))


@pytest.mark.parametrize("kind", ["eofs", "optimals"])
def test_solve_against_dense(kind, s2k_host):
    """The CPU configuration (8 nodes, ncv = 24, atol = 1e-10): ``|theta_j - theta_j^dense| <= 1e-10 theta_1`` (the bound
    ``test_gpu_resolvent.py`` uses for this iteration at this tolerance), the modes orthonormal in the weight to 1e-10, the residual
    ``||S e_j - theta_j e_j|| <= 1e-8 theta_1`` in the weight's norm with ``S`` applied by SuperLU (the resolvent's residual
    precedent), the entry of largest magnitude positive, and the rows of ``spectrum`` summing to ``variances`` to 1e-8 relative."""
    res = solved(kind)
    dense = np.array(GOLDEN[kind][:4])
    Q = s2k_host.weight(kind)
    got, X = res.variances, res.modes
    err = np.abs(got - dense).max() / dense[0] if len(got) == 4 else np.inf
    orth = np.abs(X.T @ (Q @ X) - np.eye(X.shape[1])).max()
    resid = max(ref.weight_norm(Q, s2k_host.apply(X[:, j], kind)[0] - got[j] * X[:, j]) for j in range(X.shape[1])) / dense[0]
    rows = np.abs(res.spectrum.sum(axis=1) - got).max() / got.min()
    print(f"{kind}: variances {got}, |theta - dense|_max / theta_1 = {err:.2e}, |X^T Q X - I|_max = {orth:.2e}, residual / theta_1 = {resid:.2e}, "
          f"spectrum rows {rows:.2e}; stats {res.stats}")
    assert len(got) == 4 and (np.diff(got) <= 0.0).all() and res.kind == kind
    assert err <= 1e-10
    assert orth <= 1e-10
    assert resid <= 1e-8
    for x in X.T:
        assert x[int(np.argmax(np.abs(x)))] > 0.0
    assert res.spectrum.shape == (4, 8) and (np.abs(res.spectrum.sum(axis=1) - got) <= 1e-8 * got).all()
    st = res.stats
    assert st["adjoint_solves"] == 8 * st["applies"] and st["forward_solves"] == 8 * st["applies"] and st["refinements"] == 0


@pytest.mark.parametrize("nodes,kind", [(3, "eofs"), (16, "eofs"), (3, "optimals")])
def test_batched_forward_solves_give_the_same_bits(nodes, kind):
    """``batch_forward=True`` against the default: variances, modes and spectrum byte for byte alike.  16 nodes fill a group of the
    batched sweeps, 3 nodes are a partial one; the optimals' forward solves are the first of a step and share one right-hand side."""
    one = solved(kind, nodes=nodes, ncv=12, num_modes=2, atol=1e-8)
    two = solved(kind, nodes=nodes, ncv=12, num_modes=2, atol=1e-8, batch_forward=True)
    assert two.stats["batch_forward"] and not one.stats["batch_forward"]
    assert len(one.variances) == 2
    for name in ("variances", "modes", "spectrum", "estimates"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    assert one.stats["applies"] == two.stats["applies"]


def test_forced_refinement():
    """Every solve with the refinement step: the eigenvalues meet the bound of ``test_solve_against_dense`` and the counts show 2N
    refined solves per step."""
    res = solved("eofs", refine=True)
    dense = np.array(GOLDEN["eofs"][:4])
    st = res.stats
    err = np.abs(res.variances - dense).max() / dense[0] if len(res.variances) == 4 else np.inf
    print(f"forced refinement: |theta - dense|_max / theta_1 = {err:.2e}; stats {st}")
    assert err <= 1e-10
    assert st["refined_adjoint"] == 8 * st["applies"] == st["adjoint_solves"]
    assert st["refined_forward"] == 8 * st["applies"] == st["forward_solves"]


def test_two_runs_give_the_same_bits():
    a, b = solved("eofs", nodes=4, ncv=12, num_modes=2, atol=1e-8, tag=0), solved("eofs", nodes=4, ncv=12, num_modes=2, atol=1e-8, tag=1)
    assert a is not b
    for name in ("variances", "modes", "spectrum", "estimates"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_create_refuses_what_it_cannot_run(hip_ctx):
    """``lsa_stochastic_create``: LSA_ERR_ARG naming the condition for a complex A, patterns that differ and a weight that is not
    positive; the memory rule through the planner with a made-up budget and the figures of the prepared analysis."""
    import lsa_hip
    from Solver.stochastic import StochasticForcingSolver, plan_factor_sets

    A, M, dA, dM = s2k_device(hip_ctx)
    om, w = ref.gauss_band(*ref.BAND, 4)

    def refused(a, m, weights, word):
        with pytest.raises(ValueError) as info:  # (how the binding reports LSA_ERR_ARG; every other status is an LsaError)
            lsa_hip.StochasticBasis(hip_ctx, a, m, 1j * om, weights, 12)
        assert not isinstance(info.value, lsa_hip.LsaError) and "lsa_stochastic_create" in str(info.value) and word in str(info.value), str(info.value)

    refused(lsa_hip.CsrMatrix.from_scipy(hip_ctx, A.astype(np.complex128)), dM, w, "A is complex")
    n = A.shape[0]
    assert A[0, n - 1] == 0.0
    other = lsa_hip.CsrMatrix.from_scipy(hip_ctx, sp.csr_matrix(M + sp.csr_matrix(([1.0], ([0], [n - 1])), shape=M.shape)))  # one entry more
    refused(dA, other, w, "one pattern")
    bad = w.copy()
    bad[2] = -bad[2]
    refused(dA, dM, bad, "weight 2")
    with pytest.raises(ValueError, match="lsa_shifted_spmm"):
        lsa_hip.shifted_spmm(hip_ctx, dA, other, 1j * om, np.zeros((n, 4), dtype=complex))
    sf = StochasticForcingSolver(*ref.case("S2k"))
    sf.solver.set_target(1j)
    sf.solver.prepare()
    ctx = sf.solver._prepared["ctx"]
    per_set, free = ctx.prepared_lu_bytes(), ctx.mem_info()[0]
    assert per_set > 0 and plan_factor_sets(16, per_set, free) == 16 * per_set
    with pytest.raises(MemoryError) as info:
        plan_factor_sets(16, per_set, 10 * per_set)
    assert str(16 * per_set) in str(info.value) and str(8 * per_set) in str(info.value)
    sf.release()
