"""GPU tests of block solves on one factorisation of the exact LU (``lsa_ndlu_solve_multi``, the multi-column sweeps of
``csrc/ndlu_multi.hip``): every column holds, bit for bit, what ``lsa_ndlu_solve`` / ``lsa_ndlu_solve_adjoint`` gives for it."""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SIGMA = 0.018 + 0.7379601143282424j  # the complex shift of the top-inverse tests

# (case, shift, vectors, numbers of right-hand sides): 1 = the solo entry, 2 / 8 = full passes, 3 = a pass and a remainder,
# 11 = passes and a remainder (real vectors 8 + 2 + 1, complex vectors 4 + 4 + 2 + 1)
CASES = {
    "S5k-complex": ("S5k", SIGMA, "c", (1, 2, 3, 8, 11)),
    "S5k-real": ("S5k", 0.05, "r", (1, 2, 3, 8, 11)),
    "S5k-real-complex-vectors": ("S5k", 0.05, "c", (1, 2, 3, 8, 11)),
    "C9k-constraints": ("C9k", -5.0, "c", (1, 2, 3, 8, 11)),  # a 3D forest: no assembled top
    "S30k-complex": ("S30k", SIGMA, "c", (8,)),               # top s = 608
}

_SETUPS = {}


def _matrix(case, sigma):
    from synthetic import fem

    es = fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    if complex(sigma).imag == 0.0:
        C = sp.csr_matrix(C.real)
    C.sort_indices()
    zd = C.diagonal() == 0  # (the 3D cases: constraint unknowns are eliminated after their neighbours)
    return C, (zd if (zd.any() and C.nnz > 60 * es.n) else None)


def _setup(hip_ctx, case, sigma, ordered):
    """The factorisation of ``case`` at ``sigma`` (kept for the module): in the elimination order of ``nd_order`` with the forest
    handed back (ORDERED sweeps, the assembled top where the forest has one), or with the library's own dissection."""
    import lsa_hip

    key = (case, complex(sigma), ordered)
    if key not in _SETUPS:
        C, flags = _matrix(case, sigma)
        sizes = perm = None
        if ordered:
            o = lsa_hip.nd_order(C, 0, constraint=flags)
            C = C[o["perm"]][:, o["perm"]].tocsr()
            C.sort_indices()
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            f = lsa_hip.NdLu(hip_ctx, dC, 0, tree={"first": o["first"], "size": o["size"], "parent": o["parent"]})
            sizes, perm = o["size"], o["perm"]
        else:
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            f = lsa_hip.NdLu(hip_ctx, dC, 0)
        _SETUPS[key] = {"f": f, "dC": dC, "C": C, "n": C.shape[0], "sizes": sizes, "perm": perm}
    return _SETUPS[key]


def _block(n, k, vectors, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return np.asfortranarray(B + 1j * rng.standard_normal((n, k)) if vectors == "c" else B)


def _solo(hip_ctx, f, B, adjoint=None):
    import lsa_hip

    X = np.empty_like(B)
    for q in range(B.shape[1]):
        x = lsa_hip.DeviceVector(hip_ctx, B.shape[0], B.dtype)
        b = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(B[:, q]))
        if adjoint is None:
            f.solve(b, x)
        else:
            f.solve_adjoint(b, x, conj=adjoint)
        X[:, q] = x.numpy()
    return X


def _multi(hip_ctx, f, B, trans="N"):
    import lsa_hip

    n, k = B.shape
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    dX = lsa_hip.DeviceVector(hip_ctx, n * k, B.dtype)
    f.solve_multi(dB, dX, k, trans=trans)
    return dX.numpy().reshape((n, k), order="F")


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "own-dissection"])
@pytest.mark.parametrize("name", list(CASES))
def test_columns_equal_solo_solves(hip_ctx, name, ordered):
    case, sigma, vectors, counts = CASES[name]
    s = _setup(hip_ctx, case, sigma, ordered)
    f, n = s["f"], s["n"]
    Ball = _block(n, max(counts), vectors, 23)
    ref = _solo(hip_ctx, f, Ball)
    for k in counts:
        B = np.asfortranarray(Ball[:, :k])
        X = _multi(hip_ctx, f, B)
        info = f.multi_info()
        for q in range(k):
            assert np.array_equal(X[:, q], ref[:, q]), (name, ordered, k, q)
        if k > 1:
            most = 4 if vectors == "c" else 8  # the library's measured choice: complex vectors in passes of at most four
            assert info["width"] == (most if k >= most else 2 if k < 4 else 4), info
            assert info["extra_bytes"] > 0 and info["launches_per_pass"] == f.info()["apply_launches"]
        res = np.linalg.norm(B - s["C"] @ X) / np.linalg.norm(B)
        print(f"{name} ordered={ordered} nrhs={k}: width {info['width']}, |B - C X|_F/|B|_F = {res:.2e}")
        assert res <= 1e-12


def test_a_case_is_wider_than_the_staging_chunk(hip_ctx):
    """The multi-chunk path of the kernels is exercised: the assembled top of S5k (739 unknowns) and of S30k (608) and the
    widest pivot block of C9k are wider than the ``NDLU_MULTI_CHUNK`` entries a workgroup stages per column at a time."""
    import lsa_hip
    from test_topinv_cpu import TOP_LIMIT, top_plan

    assert lsa_hip.NDLU_MULTI_CHUNK % 256 == 0 and lsa_hip.NDLU_MULTI_MAX * lsa_hip.NDLU_MULTI_CHUNK * 8 <= 64 * 1024
    C, flags = _matrix("S5k", SIGMA)
    plan = top_plan(lsa_hip.NdAnalysis(C, 0, constraint=flags).export_tables(), TOP_LIMIT)
    assert plan is not None and plan[2] > lsa_hip.NDLU_MULTI_CHUNK
    sizes = _setup(hip_ctx, "C9k", -5.0, True)["sizes"]
    print(f"S5k top: {plan[2]} unknowns; C9k widest pivot block: {int(sizes.max())}; chunk {lsa_hip.NDLU_MULTI_CHUNK}")
    assert int(sizes.max()) > lsa_hip.NDLU_MULTI_CHUNK


def test_buffer_hygiene_on_one_factorisation(hip_ctx):
    """Solo and multi solves, real and complex vectors, refactorisation, in place and padded blocks on ONE factorisation with
    real factors: the sweep buffers of the extra columns (their slot tables above all) never leak from one solve into the next."""
    import lsa_hip

    s = _setup(hip_ctx, "S5k", 0.05, True)
    f, n = s["f"], s["n"]
    Br, Bc = _block(n, 5, "r", 5), _block(n, 5, "c", 6)
    # solo -> multi -> solo -> multi
    solo1 = _solo(hip_ctx, f, Br)
    multi1 = _multi(hip_ctx, f, Br)
    solo2 = _solo(hip_ctx, f, Br)
    multi2 = _multi(hip_ctx, f, Br)
    assert f.multi_info()["width"] == 4
    for X in (multi1, solo2, multi2):
        assert np.array_equal(X, solo1)
    # real vectors, complex vectors, and back: the slot tables are indexed in units of the vector scalar
    multi_c = _multi(hip_ctx, f, Bc)
    multi_r = _multi(hip_ctx, f, Br)
    multi_c2 = _multi(hip_ctx, f, Bc)
    assert np.array_equal(multi_r, solo1)
    solo_c = _solo(hip_ctx, f, Bc)
    assert np.array_equal(multi_c, solo_c) and np.array_equal(multi_c2, solo_c)
    assert np.array_equal(_multi(hip_ctx, f, Br), _solo(hip_ctx, f, Br))
    # in place equals out of place
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, Bc.reshape(-1, order="F"))
    f.solve_multi(dB, dB, 5)
    assert np.array_equal(dB.numpy().reshape((n, 5), order="F"), solo_c)
    # leading dimensions above n, NaN in the padding: not read from B, untouched in X
    ldb, ldx, k = n + 3, n + 5, 5
    hb = np.full(ldb * k, np.nan + 1j * np.nan)
    hx = np.full(ldx * k, 7.0 - 3.0j)
    for q in range(k):
        hb[q * ldb:q * ldb + n] = Bc[:, q]
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, hb)
    dX = lsa_hip.DeviceVector.from_numpy(hip_ctx, hx)
    f.solve_multi(dB, dX, k, ldb=ldb, ldx=ldx)
    out = dX.numpy()
    for q in range(k):
        assert np.array_equal(out[q * ldx:q * ldx + n], solo_c[:, q])
        pad = out[q * ldx + n:(q + 1) * ldx]
        assert np.all(pad == 7.0 - 3.0j)
    # after a refactorisation to a second shift, multi equals solo (and the first shift's answers come back with it)
    C2 = _matrix("S5k", 0.06)[0][s["perm"]][:, s["perm"]].tocsr()
    C2.sort_indices()
    d2 = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C2)
    f.refactor(d2)
    try:
        X2 = _multi(hip_ctx, f, Bc)
        assert np.array_equal(X2, _solo(hip_ctx, f, Bc))
        assert np.linalg.norm(Bc - C2 @ X2) <= 1e-12 * np.linalg.norm(Bc)
        assert not np.array_equal(X2, solo_c)
    finally:
        f.refactor(s["dC"])
    assert np.array_equal(_multi(hip_ctx, f, Bc), solo_c)


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "own-dissection"])
def test_transposed_block_solves_equal_adjoint_solves(hip_ctx, ordered):
    s = _setup(hip_ctx, "S5k", SIGMA, ordered)
    f, n = s["f"], s["n"]
    B = _block(n, 3, "c", 31)
    for trans, conj in (("T", False), ("H", True)):
        X = _multi(hip_ctx, f, B, trans=trans)
        assert f.multi_info()["width"] == 1  # the existing transposed sweeps, column by column
        assert np.array_equal(X, _solo(hip_ctx, f, B, adjoint=conj))
        op = s["C"].conj().T if conj else s["C"].T
        assert np.linalg.norm(B - op @ X) <= 1e-12 * np.linalg.norm(B)


def test_argument_errors_leave_x_unchanged(hip_ctx):
    import lsa_hip

    s = _setup(hip_ctx, "S5k", SIGMA, True)   # complex factors
    r = _setup(hip_ctx, "S5k", 0.05, True)    # real factors
    f, n = s["f"], s["n"]
    k = 3
    mark = np.full((n + 2) * k, 1.5 - 2.5j)
    dX = lsa_hip.DeviceVector.from_numpy(hip_ctx, mark)
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, _block(n + 2, k, "c", 3).reshape(-1, order="F"))
    short = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ones(n * k - 1, dtype=np.complex128))
    realB = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ones(n * k))
    realX = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * k, 4.25))
    bad = [
        dict(B=dB, X=dX, nrhs=0),                      # nrhs < 1
        dict(B=dB, X=dX, nrhs=-2),
        dict(B=dB, X=dX, nrhs=k, ldb=n - 1),           # ld < n
        dict(B=dB, X=dX, nrhs=k, ldx=n - 1),
        dict(B=short, X=dX, nrhs=k),                   # a block shorter than ld (nrhs - 1) + n
        dict(B=dB, X=dX, nrhs=k + 1, ldx=n + 2),
        dict(B=realB, X=dX, nrhs=k),                   # mixed vector dtypes
        dict(B=dX, X=dX, nrhs=k, ldb=n, ldx=n + 1),    # an overlap that is not the in-place form
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            f.solve_multi(kw.pop("B"), kw.pop("X"), kw.pop("nrhs"), **kw)
        assert np.array_equal(dX.numpy(), mark)
    with pytest.raises(ValueError):                    # complex factors with real vectors
        f.solve_multi(realB, realX, k)
    assert np.all(realX.numpy() == 4.25)
    with pytest.raises(ValueError):
        f.solve_multi(dB, dX, k, trans="C")
    assert np.array_equal(dX.numpy(), mark)
    # ... and the same block is fine on real factors with real vectors, where nothing above applies
    r["f"].solve_multi(realB, realX, k)
    assert np.all(np.isfinite(realX.numpy())) and not np.all(realX.numpy() == 4.25)


def test_time_solve_multi_reports_a_duration(hip_ctx):
    import lsa_hip

    s = _setup(hip_ctx, "S5k", SIGMA, True)
    f, n = s["f"], s["n"]
    B = _block(n, 4, "c", 9)
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    dX = lsa_hip.DeviceVector(hip_ctx, n * 4, np.complex128)
    ms = f.time_solve_multi(dB, dX, 4, iters=3)
    assert ms > 0.0 and f.multi_info()["width"] == 4
    assert np.array_equal(dX.numpy().reshape((n, 4), order="F"), _solo(hip_ctx, f, B))
    with pytest.raises(ValueError):
        f.time_solve_multi(dB, dB, 4, iters=3)
