"""GPU tests of transposed and adjoint block solves in wide passes (``lsa_ndlu_set_multi_transposed``, the kernel
``nd_sweepT_multi_kernel`` of ``csrc/ndlu_multi.hip``): with the switch on every column of ``lsa_ndlu_solve_multi(trans = T / H)``
holds, bit for bit, what ``lsa_ndlu_solve_adjoint`` gives for it, and so do the front ends built on it (``iKSP.block_adjoint``,
``ResolventSolver(block_forcings=True)``).  Set-up helpers after ``test_gpu_multi_rhs.py``."""

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SIGMA = 0.018 + 0.7379601143282424j  # the complex shift of the top-inverse tests

# (case, shift, vectors, numbers of right-hand sides): 2 / 4 / 8 = full passes, 3 / 5 = a pass and a solo remainder, 11 = passes
# and remainders (real vectors 8 + 2 + 1, complex vectors 4 + 4 + 2 + 1)
CASES = {
    "S5k-complex": ("S5k", SIGMA, "c", (2, 3, 4, 5, 11)),
    "S5k-real": ("S5k", 0.05, "r", (2, 3, 8, 11)),
    "S5k-real-complex-vectors": ("S5k", 0.05, "c", (4, 5)),
    "C9k-constraints": ("C9k", -5.0, "c", (3, 8)),  # a 3D forest with constraints: pivot blocks and boundaries of several chunks
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
    handed back, or with the library's own dissection."""
    import lsa_hip

    key = (case, complex(sigma), ordered)
    if key not in _SETUPS:
        C, flags = _matrix(case, sigma)
        sizes = perm = fronts = None
        if ordered:
            o = lsa_hip.nd_order(C, 0, constraint=flags)
            C = C[o["perm"]][:, o["perm"]].tocsr()
            C.sort_indices()
            tree = {"first": o["first"], "size": o["size"], "parent": o["parent"]}
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            f = lsa_hip.NdLu(hip_ctx, dC, 0, tree=tree)
            sizes, perm = o["size"], o["perm"]
            fronts = lsa_hip.NdAnalysis(C, 0, tree=tree).export()["front_size"]
        else:
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            f = lsa_hip.NdLu(hip_ctx, dC, 0)
        _SETUPS[key] = {"f": f, "dC": dC, "C": C, "n": C.shape[0], "sizes": sizes, "perm": perm, "fronts": fronts}
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


def _width(k, vectors):
    most = 4 if vectors == "c" else 8  # the library's cap: complex vectors in passes of at most four
    return most if k >= most else 2 if k < 4 else 4


@pytest.mark.parametrize("trans", ["T", "H"])
@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "own-dissection"])
@pytest.mark.parametrize("name", list(CASES))
def test_columns_equal_solo_adjoint_solves(hip_ctx, name, ordered, trans):
    case, sigma, vectors, counts = CASES[name]
    s = _setup(hip_ctx, case, sigma, ordered)
    f, n = s["f"], s["n"]
    conj = trans == "H"
    op = s["C"].conj().T if conj else s["C"].T
    Ball = _block(n, max(counts), vectors, 29)
    ref = _solo(hip_ctx, f, Ball, adjoint=conj)
    try:
        for k in counts:
            B = np.asfortranarray(Ball[:, :k])
            f.set_multi_transposed(True)
            X = _multi(hip_ctx, f, B, trans=trans)
            info = f.multi_info()
            for q in range(k):
                assert np.array_equal(X[:, q], ref[:, q]), (name, ordered, trans, k, q)
            assert info["width"] == _width(k, vectors) and info["width"] > 1, info
            res = np.linalg.norm(B - op @ X) / np.linalg.norm(B)
            print(f"{name} ordered={ordered} trans={trans} nrhs={k}: width {info['width']}, |B - op(C) X|_F/|B|_F = {res:.2e}")
            assert res <= 1e-12
            f.set_multi_transposed(False)
            X = _multi(hip_ctx, f, B, trans=trans)
            assert f.multi_info()["width"] == 1
            assert np.array_equal(X, ref[:, :k])
    finally:
        f.set_multi_transposed(False)


def test_c9k_stages_several_chunks_in_both_sweeps(hip_ctx):
    """The widest pivot block of C9k (the rows the upward sweep sums over) and its widest boundary (those of the downward sweep) are
    longer than the ``NDLU_MULTI_CHUNK`` entries a workgroup stages per column at a time."""
    import lsa_hip

    s = _setup(hip_ctx, "C9k", -5.0, True)
    sizes, fronts = s["sizes"], s["fronts"]
    print(f"C9k widest pivot block {int(sizes.max())}, widest boundary {int((fronts - sizes).max())}; chunk {lsa_hip.NDLU_MULTI_CHUNK}")
    assert lsa_hip.NDLU_MULTI_CHUNK % 16 == 0
    assert int(sizes.max()) > lsa_hip.NDLU_MULTI_CHUNK
    assert int((fronts - sizes).max()) > lsa_hip.NDLU_MULTI_CHUNK


def test_buffer_hygiene_on_one_factorisation(hip_ctx):
    """Forward and transposed block solves, solo solves in both directions, real and complex vectors, in place and padded blocks and
    a refactorisation on ONE factorisation with real factors: every result equals its solo counterpart, and the forward results do
    not move."""
    import lsa_hip

    s = _setup(hip_ctx, "S5k", 0.05, True)
    f, n = s["f"], s["n"]
    Br, Bc = _block(n, 5, "r", 7), _block(n, 5, "c", 8)
    fwd_r, fwd_c = _solo(hip_ctx, f, Br), _solo(hip_ctx, f, Bc)
    adj_r, adj_c = _solo(hip_ctx, f, Br, adjoint=True), _solo(hip_ctx, f, Bc, adjoint=True)
    f.set_multi_transposed(True)
    try:
        # forward multi, transposed multi, solo adjoint, solo forward, transposed multi again
        assert np.array_equal(_multi(hip_ctx, f, Br), fwd_r)
        assert np.array_equal(_multi(hip_ctx, f, Br, trans="H"), adj_r)
        assert f.multi_info()["width"] == 4
        assert np.array_equal(_solo(hip_ctx, f, Br, adjoint=True), adj_r)
        assert np.array_equal(_solo(hip_ctx, f, Br), fwd_r)
        assert np.array_equal(_multi(hip_ctx, f, Br, trans="T"), adj_r)
        # real vectors, complex vectors and back, forward solves in between
        assert np.array_equal(_multi(hip_ctx, f, Bc, trans="H"), adj_c)
        assert np.array_equal(_multi(hip_ctx, f, Bc), fwd_c)
        assert np.array_equal(_multi(hip_ctx, f, Br, trans="H"), adj_r)
        assert np.array_equal(_multi(hip_ctx, f, Br), fwd_r)
        assert np.array_equal(_multi(hip_ctx, f, Bc, trans="T"), adj_c)
        assert np.array_equal(_solo(hip_ctx, f, Bc), fwd_c)
        # in place equals out of place
        dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, Bc.reshape(-1, order="F"))
        f.solve_multi(dB, dB, 5, trans="H")
        assert np.array_equal(dB.numpy().reshape((n, 5), order="F"), adj_c)
        # leading dimensions above n, NaN in B's padding (not read), a marker in X's (untouched)
        ldb, ldx, k = n + 3, n + 5, 5
        hb = np.full(ldb * k, np.nan + 1j * np.nan)
        hx = np.full(ldx * k, 7.0 - 3.0j)
        for q in range(k):
            hb[q * ldb:q * ldb + n] = Bc[:, q]
        dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, hb)
        dX = lsa_hip.DeviceVector.from_numpy(hip_ctx, hx)
        f.solve_multi(dB, dX, k, ldb=ldb, ldx=ldx, trans="H")
        assert f.multi_info()["width"] == 4
        out = dX.numpy()
        for q in range(k):
            assert np.array_equal(out[q * ldx:q * ldx + n], adj_c[:, q])
            assert np.all(out[q * ldx + n:(q + 1) * ldx] == 7.0 - 3.0j)
        # a refactorisation to a second shift and back
        C2 = _matrix("S5k", 0.06)[0][s["perm"]][:, s["perm"]].tocsr()
        C2.sort_indices()
        d2 = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C2)
        f.refactor(d2)
        try:
            X2 = _multi(hip_ctx, f, Bc, trans="H")
            assert f.multi_info()["width"] == 4
            assert np.array_equal(X2, _solo(hip_ctx, f, Bc, adjoint=True))
            assert np.linalg.norm(Bc - C2.T @ X2) <= 1e-12 * np.linalg.norm(Bc)
            assert not np.array_equal(X2, adj_c)
            assert np.array_equal(_multi(hip_ctx, f, Bc), _solo(hip_ctx, f, Bc))
        finally:
            f.refactor(s["dC"])
        assert np.array_equal(_multi(hip_ctx, f, Bc, trans="H"), adj_c)
        assert np.array_equal(_multi(hip_ctx, f, Bc), fwd_c)
        assert np.array_equal(_multi(hip_ctx, f, Br), fwd_r)
    finally:
        f.set_multi_transposed(False)


def test_iksp_block_adjoint_keeps_every_bit():
    from Solver.utils import KSPType, PreconditionerType, iKSP

    C = _matrix("S5k", SIGMA)[0]
    n = C.shape[0]
    B = _block(n, 5, "c", 13)
    ksp = iKSP(C)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(rtol=1e-12)
    off = ksp.solve_many(B, adjoint=True)
    assert ksp.stats["multi_width"] == 1
    ksp.block_adjoint = True
    on = ksp.solve_many(B, adjoint=True)
    assert ksp.stats["multi_width"] > 1
    assert np.array_equal(on, off)
    assert np.linalg.norm(B - C.conj().T @ on) <= 1e-12 * np.linalg.norm(B)
    ksp.block_adjoint = False
    assert np.array_equal(ksp.solve_many(B, adjoint=True), off)
    assert ksp.stats["multi_width"] == 1
    assert ksp.stats["factorisations"] == 1
    ksp.reset()


def test_resolvent_block_forcings_keep_every_bit():
    """S2k, num_modes 4, ncv 12, atol 1e-10 (the front-end solve of ``test_gpu_resolvent.py``) with the forcings' adjoint solves one by
    one and as one block solve."""
    import resolvent_reference as ref
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case("S2k")
    cfg = ResolventConfig(num_modes=4, ncv=12, atol=1e-10)
    out = []
    for flag in (False, True):
        rs = ResolventSolver(A, M, cfg, block_forcings=flag)
        out.append(rs.solve(ref.OMEGA_TARGET))
        rs.release()
    off, on = out
    assert len(off.gains) == 4
    assert np.array_equal(on.gains, off.gains)
    assert np.array_equal(on.responses, off.responses)
    assert np.array_equal(on.forcings, off.forcings)
    for key in ("adjoint_solves", "refined_adjoint", "forward_solves"):
        assert on.stats[key] == off.stats[key], key
    assert on.stats["max_rel_res"] == off.stats["max_rel_res"]


def test_time_solve_multi_adjoint_reports_a_duration(hip_ctx):
    import lsa_hip

    s = _setup(hip_ctx, "S5k", SIGMA, True)
    f, n = s["f"], s["n"]
    B = _block(n, 4, "c", 9)
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    dX = lsa_hip.DeviceVector(hip_ctx, n * 4, np.complex128)
    f.set_multi_transposed(True)
    try:
        ms = f.time_solve_multi(dB, dX, 4, iters=3, trans="H")
        assert ms > 0.0 and f.multi_info()["width"] == 4
    finally:
        f.set_multi_transposed(False)
    assert np.array_equal(dX.numpy().reshape((n, 4), order="F"), _solo(hip_ctx, f, B, adjoint=True))
