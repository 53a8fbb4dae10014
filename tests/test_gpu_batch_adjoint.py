"""GPU tests of the batched transposed sweeps of the exact LU (``lsa_ndlu_solve_batch_adjoint``, ``NdLu.solve_batch(trans=)``) and of the
batched transposed SpMV (``lsa_spmv_transpose_batch``): every problem of a batch gets, bit for bit, what it gets alone."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

# (set-up as in test_gpu_batch.py) tabulated targets of the harness sweep (lsa-fw_amd/examples/eigenvalues.py), Re = 40, 45, ..., 90
REYNOLDS = tuple(range(40, 91, 5))
TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j), (0.03 + 0.742986662573986j),
           (0.05 + 0.744243299635422j), (0.061 + 0.7461282552275759j), (0.072 + 0.7461282552275759j), (0.085 + 0.744557458900781j),
           (0.09 + 0.742986662573986j), (0.1 + 0.7398450699203962j), (0.115 + 0.7351326809400116j))

_CASES = {}
_FACTORS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_factors():
    yield
    _FACTORS.clear()


def _case(name, re):
    from synthetic import fem

    if (name, re) not in _CASES:
        _CASES[(name, re)] = fem.cylinder_case(name, re=float(re))
    return _CASES[(name, re)]


def _shifted(name, re_, sigma):
    es = _case(name, re_)
    return sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)


def _factors(hip_ctx, name, res, targets):
    """``[(NdLu, device C, host C)]``, one factorisation per (Reynolds number, shift); made once per process."""
    import lsa_hip

    key = (name, tuple(res), tuple(targets))
    if key not in _FACTORS:
        out = []
        for re_, sigma in zip(res, targets):
            C = _shifted(name, re_, sigma)
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            out.append((lsa_hip.NdLu(hip_ctx, dC, 0), dC, C))
        _FACTORS[key] = out
    return _FACTORS[key]


def _sets(hip_ctx, J, shifts):
    name, res = ("S2k", REYNOLDS[:1] * J) if shifts == "complex_S2k" else ("S5k", REYNOLDS[:J])
    if shifts == "complex_S2k":
        targets = tuple(TARGETS[0] + 0.01 * j * (1 + 1j) for j in range(J))
    else:
        targets = TARGETS[:J] if shifts == "complex" else tuple(0.05 + 0.01 * j for j in range(J))
    assert len(set(targets)) == J == len(res)
    return _factors(hip_ctx, name, res, targets)


def _rhs(n, J, vdtype, seed=11):
    rng = np.random.default_rng(seed)
    bs = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(J)]
    return [b.real.copy() for b in bs] if vdtype is np.float64 else bs


def _solo_adjoint(hip_ctx, fs, bs, vdtype, trans):
    import lsa_hip

    out = []
    for (f, _, _), b in zip(fs, bs):
        x = lsa_hip.DeviceVector(hip_ctx, len(b), vdtype)
        f.solve_adjoint(lsa_hip.DeviceVector.from_numpy(hip_ctx, b), x, conj=(trans == "H"))
        out.append(x.numpy())
    return out


@pytest.mark.parametrize("J,shifts,vdtype,trans", [(1, "complex", np.complex128, "H"), (3, "complex", np.complex128, "H"),
                                                   (3, "complex", np.complex128, "T"), (3, "real", np.complex128, "H"),
                                                   (3, "real", np.float64, "T"), (16, "complex_S2k", np.complex128, "H")])
def test_ndlu_solve_batch_adjoint_equals_solo_solves(hip_ctx, J, shifts, vdtype, trans):
    """Complex factors with ``H`` and ``T``, real factors with complex vectors (``H`` is the transposed solve there) and with real
    vectors: each instance of the batched transposed sweeps (the kernels at the batch's pointer capacity) against
    ``lsa_ndlu_solve_adjoint`` per factor set (the same kernels at capacity one).  S5k at three Reynolds numbers: the factors differ in
    value and share the pattern.  J = 16 fills the pointer struct to its last slot: sixteen distinct complex shifts of S2k."""
    import lsa_hip

    fs = _sets(hip_ctx, J, shifts)
    n = fs[0][1].shape[0]
    bs = _rhs(n, J, vdtype)
    solo = _solo_adjoint(hip_ctx, fs, bs, vdtype, trans)
    dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
    dxs = [lsa_hip.DeviceVector(hip_ctx, n, vdtype) for _ in range(J)]
    lsa_hip.NdLu.solve_batch([f for f, _, _ in fs], dbs, dxs, trans=trans)
    for x, ref in zip(dxs, solo):
        assert np.array_equal(x.numpy(), ref)
    # in place (x = b), and a second time on fresh right-hand sides: the same bits again
    lsa_hip.NdLu.solve_batch([f for f, _, _ in fs], dbs, dbs, trans=trans)
    for x, ref in zip(dbs, solo):
        assert np.array_equal(x.numpy(), ref)
    dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
    lsa_hip.NdLu.solve_batch([f for f, _, _ in fs], dbs, dxs, trans=trans)
    for x, ref in zip(dxs, solo):
        assert np.array_equal(x.numpy(), ref)


def test_batched_adjoint_residual_against_superlu(hip_ctx):
    """An anchor that does not pass through the solo kernel: for the J = 3 complex case the host residual ``||C_z^H x_z - b_z||_2`` of the
    batched solve is at most 10 x the residual ``scipy.sparse.linalg.splu(C_z^H)`` leaves for the same ``b_z``.  Both are backward-stable
    eliminations with different pivot orders: ten covers the difference of their growth factors and admits no wrong block."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    n = fs[0][1].shape[0]
    bs = _rhs(n, 3, np.complex128)
    dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
    dxs = [lsa_hip.DeviceVector(hip_ctx, n, np.complex128) for _ in range(3)]
    lsa_hip.NdLu.solve_batch([f for f, _, _ in fs], dbs, dxs, trans="H")
    pairs = []
    for (_, _, C), b, dx in zip(fs, bs, dxs):
        CH = sp.csc_matrix(C.conj().T)
        ours = float(np.linalg.norm(CH @ dx.numpy() - b))
        theirs = float(np.linalg.norm(CH @ spla.splu(CH).solve(b) - b))
        pairs.append((ours, theirs))
    print("||C^H x - b||_2 (batched sweeps, SuperLU): " + ", ".join(f"({o:.3e}, {t:.3e})" for o, t in pairs) + f"; ||b||_2 = {np.linalg.norm(bs[0]):.3e}")
    for ours, theirs in pairs:
        assert ours <= 10.0 * theirs


def test_batched_adjoint_leaves_the_other_solves_their_bits(hip_ctx):
    """The update vectors (``d_ubuf``) serve both directions: after a batched ``H`` solve on three sets, a batched ``N`` solve, a solo
    ``solve`` and a solo ``solve_adjoint`` on the same sets give the bits they gave before it."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    n = fs[0][1].shape[0]
    bs = _rhs(n, 3, np.complex128, seed=12)

    def three():
        dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
        dxs = [lsa_hip.DeviceVector(hip_ctx, n, np.complex128) for _ in range(3)]
        lsa_hip.NdLu.solve_batch(factors, dbs, dxs)
        out = [x.numpy() for x in dxs]
        for f, b in zip(factors, dbs):
            x = lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
            f.solve(b, x)
            out.append(x.numpy())
        return out + _solo_adjoint(hip_ctx, fs, bs, np.complex128, "H")

    before = three()
    dbs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, b) for b in bs]
    dxs = [lsa_hip.DeviceVector(hip_ctx, n, np.complex128) for _ in range(3)]
    lsa_hip.NdLu.solve_batch(factors, dbs, dxs, trans="H")
    after = three()
    assert len(before) == len(after) == 9
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for x, ref in zip(dxs, before[6:]):
        assert np.array_equal(x.numpy(), ref)


def test_ndlu_solve_batch_adjoint_rejects_what_it_cannot_run(hip_ctx):
    import lsa_hip

    (f5, d5, _), = _factors(hip_ctx, "S5k", REYNOLDS[:1], TARGETS[:1])
    (f2, d2, _), = _factors(hip_ctx, "S2k", REYNOLDS[:1], TARGETS[:1])
    (fr, dr, _), = _factors(hip_ctx, "S5k", REYNOLDS[1:2], (0.05,))  # real shift: real factors
    n5, n2 = d5.shape[0], d2.shape[0]
    v5 = [lsa_hip.DeviceVector(hip_ctx, n5, np.complex128) for _ in range(4)]
    v2 = lsa_hip.DeviceVector(hip_ctx, n2, np.complex128)
    # (LSA_ERR_ARG reaches Python as ValueError)
    with pytest.raises(ValueError, match="lsa_ndlu_solve_batch_adjoint.*same analysis"):
        lsa_hip.NdLu.solve_batch([f5, f2], [v5[0], v2], [v5[1], v2], trans="H")
    with pytest.raises(ValueError, match="lsa_ndlu_solve_batch_adjoint.*same analysis"):
        lsa_hip.NdLu.solve_batch([f5, fr], v5[:2], v5[2:], trans="H")
    with pytest.raises(ValueError, match="lsa_ndlu_solve_batch_adjoint.*share a factorisation"):
        lsa_hip.NdLu.solve_batch([f5, f5], v5[:2], v5[2:], trans="T")
    with pytest.raises(ValueError, match="at most 16"):
        lsa_hip.NdLu.solve_batch([f5] * 17, v5[:1] * 17, v5[1:2] * 17, trans="H")
    with pytest.raises(ValueError, match="trans must be"):
        lsa_hip.NdLu.solve_batch([f5], v5[:1], v5[1:2], trans="X")


# ---- the batched transposed SpMV ---------------------------------------------------------------------------------------------

def _s2k_shifted_matrices(hip_ctx, J, values):
    import lsa_hip

    shifts = [TARGETS[0] + 0.01 * j * (1 + 1j) for j in range(J)] if values == "complex" else [0.05 + 0.01 * j for j in range(J)]
    return [lsa_hip.CsrMatrix.from_scipy(hip_ctx, _shifted("S2k", REYNOLDS[0], s)) for s in shifts]


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("values", ["complex", "real"])
@pytest.mark.parametrize("J", [1, 3, 16])
def test_spmv_transpose_batch_equals_solo_products(hip_ctx, J, values, conj):
    """``lsa_spmv_transpose_batch`` on J shifted matrices of S2k (complex values, and real values with complex vectors) against
    ``lsa_spmv_transpose`` per matrix; J = 16 fills the pointer struct."""
    import lsa_hip

    mats = _s2k_shifted_matrices(hip_ctx, J, values)
    assert mats[0].dtype == (np.complex128 if values == "complex" else np.float64)
    n = mats[0].shape[0]
    rng = np.random.default_rng(J)
    xs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, rng.standard_normal(n) + 1j * rng.standard_normal(n)) for _ in range(J)]
    solo = []
    for m, x in zip(mats, xs):
        y = lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
        m.rmatvec(x, y, conj=conj)
        solo.append(y.numpy())
    ys = [lsa_hip.DeviceVector(hip_ctx, n, np.complex128) for _ in range(J)]
    lsa_hip.CsrMatrix.spmv_transpose_batch(mats, xs, ys, conj=conj)
    for y, ref in zip(ys, solo):
        assert np.abs(ref).max() > 0.0
        assert np.array_equal(y.numpy(), ref)


def test_spmv_transpose_batch_rejects_another_pattern(hip_ctx):
    import lsa_hip

    m2, = _s2k_shifted_matrices(hip_ctx, 1, "complex")
    m5 = lsa_hip.CsrMatrix.from_scipy(hip_ctx, _shifted("S5k", REYNOLDS[0], TARGETS[0]))
    v2 = [lsa_hip.DeviceVector(hip_ctx, m2.shape[0], np.complex128) for _ in range(2)]
    v5 = [lsa_hip.DeviceVector(hip_ctx, m5.shape[0], np.complex128) for _ in range(2)]
    with pytest.raises(ValueError, match=r"spmv_transpose_batch: matrix 1 has n = "):
        lsa_hip.CsrMatrix.spmv_transpose_batch([m2, m5], [v2[0], v5[0]], [v2[1], v5[1]])
